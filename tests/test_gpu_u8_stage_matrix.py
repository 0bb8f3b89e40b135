"""The filters on the u8 outputs (csrc/isp_sharpen.hip, isp_local_contrast.hip, isp_chroma_denoise.hip, isp_luma_denoise.hip,
isp_color_lut.hip, isp_u8_stage.hip and the front end they share in csrc/isp_api.hip), instance by instance against their
NumPy restatements (tests/sharpen_ref.py, local_contrast_ref.py, chroma_denoise_ref.py, luma_denoise_ref.py,
color_lut_ref.py).  Every contract here is an integer contract: every comparison is bit for bit.

A. No GPU: the instance table is the cross product it claims and its 25 kernel names are the stage kernels of
   profiles/u8_front_end_resources.txt; the constants the shapes rest on are the ones the sources state; every case id of
   B to E together names every kernel; and - on the restatements alone - no generated case is vacuous: a reference
   differs from its input, a local contrast tiling has a tile edge in x at a multiple of 4 and one that is not, and the
   "extremes" inputs of D drive the deltas to the largest magnitude the contract of DESIGN.md 3 admits at that setting
   (computed from the contract) and, where the contract clamps at all, past 0 and past 255.
B. Every instance at the seams of the dword path (W % 4 == 0 and 4-byte aligned images) and at their byte-path twins,
   through the public functions, which allocate an aligned destination: W = 4 and 8 (stage_luma clamps every staged group
   to the row's one or two groups), H < 2 R + 1, exactly one 128 x 64 tile, a second tile row of one row beside a second
   tile column of one group, a tile not filled.  Local contrast runs every shape with tiles (1, 1) and with a tiling whose
   tile edges cut 4-pixel groups (hist_kernel's masked groups); the colour LUT is forced through each of its three
   instances at one chunk of that instance, one chunk +- 4 pixels and +- 1 pixel.  Two settings per stage from the feature
   tests' lists, random bytes.  The untouched plane of a planar result is compared with the rest.
C. The alignment fork through the C ABI, for all ten batch entry points (the colour LUT's _path twin once per instance):
   the source one byte off, the destination two bytes off, both off (3 and 1) - each equal to the aligned call
   and to the reference, inside buffers of sentinel bytes that must come back untouched - and, for the stages that run in
   place, in place at offsets 0 and 1.  Local contrast with the destination alone off is "histogram on dwords, apply on
   bytes".
D. The saturating write-back (add_sat4, pair) at its bounds: fields of 0 with isolated 255 pixels (the four corners, both
   sides of the tile seams at column 128 and row 64, the first and the last column of a thread's 4-pixel group), their
   inverse, and a 0 / 255 checkerboard, at the settings with the largest deltas, dword and byte path, all radii.
   Where the prescribed bytes cannot move a stage the case is replaced, not dropped: the RGB dots alternate white, red and
   cyan (a luma delta saturates a channel only where the channels differ); chroma noise reduction, which leaves grey as
   it is and works on 2 x 2 cells, takes blue / yellow cells (RGB) and dots in the U and V planes (planar).  The planar
   forms of the three stages with evenness rules take 66 rows where the RGB form takes 65.  The planar forms of luma and
   chroma noise reduction and of local contrast and the colour LUT cannot leave 0 .. 255 before the clamp (their output
   lies between the input and a mean, an equalised luma or a table entry): for them only the delta's bound is asserted.
E. The plane copy beyond its first sweep: an identity (chroma noise reduction at strength 0) on a planar image whose Y
   plane is larger than the 2048 blocks x 256 threads x 16 bytes of one sweep, compared on the device; its byte arm at
   2 x 6 and from an odd base at 64 x 128.
F. Every subset of the five stages through the ISP (ISP._finished): the 32 subsets on Camera16.tonemap_reinhard, the 16
   without the LUT on tonemap_reinhard_yuv420, the full set on Camera32, and a walk through set(); the references composed
   in _finished's order on the outputs of the same camera with every stage off, and exactly the subset's entry points
   called.
G. The overlap rule of the front end, on the device: every entry point refuses a destination shifted into its own source
   and a destination that is another image's source, and launches nothing (tests/test_u8_stage_errors_cpu.py has the
   texts).  An overlapping call is never run through a kernel.

Left to the feature tests (tests/test_gpu_sharpen.py, _local_contrast, _chroma_denoise, _luma_denoise, _color_lut): the
134 x 264 and 131 x 261 shapes of the `interior` arm, the scene inputs, every other setting, the containers, the second
launch group at 33 images, graph capture and the full-size images.  Not reached by name here: nothing of the 26 kernels;
u8::copy_bytes_kernel runs behind every planar case of B to D as well.  profiles/u8_stage_matrix_mutations.txt records the
deliberate edits of the library these tests were run against."""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import chroma_denoise_ref as C
from tests import color_lut_ref as CL
from tests import local_contrast_ref as R
from tests import luma_denoise_ref as Y
from tests import sharpen_ref as S
from tests.test_gpu_chroma_denoise import SETTINGS as CDN_SETTINGS
from tests.test_gpu_color_lut import GLOBAL, LDS, abi
from tests.test_gpu_local_contrast import CLIPS as LC_CLIPS, STRENGTHS as LC_STRENGTHS
from tests.test_gpu_luma_denoise import (CDN_ARGS, LC_ARGS, LDN_ARGS, LUT_N, LUT_STRENGTH, SETTINGS as YDN_SETTINGS, SHARP_ARGS,
                                         frames_of)
from tests.test_gpu_sharpen import SETTINGS as SHP_SETTINGS
from tests.util import SENTINEL, _count_calls, assert_exact

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taichi_image_amd", "csrc")

# ---- the instances -------------------------------------------------------------------------------------------------------
FORMS = ("rgb", "yuv")
RADII = {"shp": (1, 2), "ydn": (1, 2, 3), "cdn": (1, 2, 3)}
KERNEL = {"shp": "shp::sharpen_kernel", "ydn": "ydn::luma_denoise_kernel", "cdn": "cdn::chroma_denoise_kernel"}
CLUT = {0: (34, GLOBAL), 4913: (17, LDS), 35937: (33, LDS)}          # the table's LDS dwords -> (N, the path that forces it)
TILE_INSTANCES = ([(s, f, r) for s in ("shp", "ydn", "cdn") for f in FORMS for r in RADII[s]]
                  + [("lc", f, None) for f in FORMS])
CLUT_INSTANCES = [("clut", "rgb", cap) for cap in CLUT]
INSTANCES = TILE_INSTANCES + CLUT_INSTANCES
COPY_KERNEL = "u8::copy_bytes_kernel"

# what the shapes rest on (test_constants_are_the_sources)
TILE_W, TILE_H, MAX_IMAGES, THREADS = 128, 64, 32, 256
COPY_BLOCKS, COPY_BYTES = 2048, 16
CLUT_PIXELS_PER_THREAD, CLUT_LDS_THREADS, CLUT_GLOBAL_THREADS = 4, 1024, 256


def kernels_of(inst):
    stage, form, r = inst
    rgb = "true" if form == "rgb" else "false"
    if stage == "lc":
        return (f"lc::hist_kernel<{rgb}>", f"lc::apply_kernel<{rgb}>", "lc::zero_kernel", "lc::lut_kernel")
    if stage == "clut":
        return (f"clut::color_lut_kernel<{r}, {CLUT_GLOBAL_THREADS if r == 0 else CLUT_LDS_THREADS}>",)
    return (f"{KERNEL[stage]}<{rgb}, {r}>",)


def name_of(inst):
    return "+".join(kernels_of(inst))


def chunk_of(cap):
    return (CLUT_GLOBAL_THREADS if cap == 0 else CLUT_LDS_THREADS) * CLUT_PIXELS_PER_THREAD


# ---- the cases -----------------------------------------------------------------------------------------------------------
RGB_DWORD = [(1, 4), (2, 8), (64, 128), (65, 132), (60, 124)]
RGB_BYTE = [(1, 3), (1, 5), (2, 7), (64, 127), (64, 129), (65, 133)]
YUV_DWORD = [(2, 4), (2, 8), (64, 128), (66, 132)]
YUV_BYTE = [(2, 6), (64, 126), (66, 130)]
SHP_YUV_BYTE = [(2, 5), (64, 129)]                                   # sharpening's planar form takes odd widths
# two settings per stage (what follows the radius in the reference's arguments): one typical, one with strength 0.5 or an
# overshoot clamp; local contrast: (clip limit, strength); the colour LUT: the strength
SETTINGS = {"shp": [(1.5, 0, None), (1.5, 0, 8)], "ydn": [(6, 14, 1.0), (6, 14, 0.5)], "cdn": [(8, 12, 1.0), (8, 12, 0.5)],
            "lc": [(None, 1.0), (2.0, 0.5)], "clut": [1.0, 0.5]}
# the settings of D: the largest deltas
EXTREME = {"shp": (8.0, 0, None), "ydn": (255, 255, 1.0), "cdn": (255, 255, 1.0), "lc": (None, 1.0), "clut": 1.0}
CLAMPING = {("shp", "rgb"), ("shp", "yuv"), ("lc", "rgb"), ("ydn", "rgb"), ("cdn", "rgb")}   # the contract's clamp can engage


def extreme_kinds(inst):
    """dots, holes and checker are 0 / 255 bytes; chroma noise reduction's RGB form, whose chroma test (4 tc = 1020) no two
    colours of 0 / 255 bytes meet exactly, adds the pair that does: blue and the green of blue's luma."""
    return ("dots", "holes", "checker") + (("peak", "trough") if inst[:2] == ("cdn", "rgb") else ())


def tile_shapes(stage, form):
    if form == "rgb":
        return [(hw, "dword") for hw in RGB_DWORD] + [(hw, "byte") for hw in RGB_BYTE]
    return ([(hw, "dword") for hw in YUV_DWORD] + [(hw, "byte") for hw in YUV_BYTE]
            + [(hw, "byte") for hw in (SHP_YUV_BYTE if stage == "shp" else [])])


def clut_shapes(cap):
    k = chunk_of(cap)
    return [((2, k // 2), "dword"), ((1, k + 4), "dword"), ((1, k - 4), "dword"), ((1, 4), "dword"), ((1, k + 1), "byte"),
            ((1, k - 1), "byte")]


B_CASES = ([(i, H, W, p) for i in TILE_INSTANCES for (H, W), p in tile_shapes(i[0], i[1])]
           + [(i, H, W, p) for i in CLUT_INSTANCES for (H, W), p in clut_shapes(i[2])])


def d_shapes(inst):
    """65 rows have no planar form where both sides must be even: those take 66"""
    return [(65, 132), (65, 133)] if inst[1] == "rgb" else [(66, 132), (66, 134)]


D_CASES = [(i, H, W) for i in INSTANCES for H, W in d_shapes(i)]

# C: (entry point, instance or None for all radii of the stage and form, stage, form)
OFFSETS = [("src+1", 1, 0), ("dst+2", 0, 2), ("src+3_dst+1", 3, 1)]
ENTRY = {("shp", "rgb"): "mi_isp_sharpen_rgb_batch", ("shp", "yuv"): "mi_isp_sharpen_yuv420_batch",
         ("lc", "rgb"): "mi_isp_local_contrast_rgb_batch", ("lc", "yuv"): "mi_isp_local_contrast_yuv420_batch",
         ("cdn", "rgb"): "mi_isp_chroma_denoise_rgb_batch", ("cdn", "yuv"): "mi_isp_chroma_denoise_yuv420_batch",
         ("ydn", "rgb"): "mi_isp_luma_denoise_rgb_batch", ("ydn", "yuv"): "mi_isp_luma_denoise_yuv420_batch",
         ("clut", "rgb"): "mi_isp_color_lut_rgb_batch"}
CLUT_PATH_ENTRY = "mi_isp_color_lut_rgb_batch_path"
ALL_ENTRIES = list(ENTRY.values()) + [CLUT_PATH_ENTRY]


def c_entries():
    """(entry point, the instances one call of the test runs) of section C"""
    out = [(ENTRY[s, f], [i for i in TILE_INSTANCES if i[:2] == (s, f)]) for s in ("shp", "lc", "cdn", "ydn") for f in FORMS]
    out.append((ENTRY["clut", "rgb"], [("clut", "rgb", 4913)]))        # the dispatcher's choice at N = 17
    out += [(CLUT_PATH_ENTRY, [i]) for i in CLUT_INSTANCES]
    return out


def c_shapes(inst):
    if inst[0] == "clut":
        k = chunk_of(inst[2])
        return [(1, k + 4), (1, k + 1)]                                # (one chunk and a thread of the next: its 4 pixels end the image)
    return [(65, 132), (65, 133)] if inst[1] == "rgb" else [(66, 132), (66, 130)]


def offset_id(stage, W, name):
    return name + ("_hist_on_dwords_apply_on_bytes" if stage == "lc" and name == "dst+2" and W % 4 == 0 else "")


C_CASES = [(e, tuple(insts), k, o) for e, insts in c_entries() for k in (0, 1) for o in OFFSETS]
C_IN_PLACE = [(e, tuple(insts), k, off) for e, insts in c_entries() if insts[0][0] in ("lc", "clut") for k in (0, 1)
              for off in (0, 1)]


def c_id(case, in_place=False):
    entry, insts, k, o = case
    H, W = c_shapes(insts[0])[k]
    kernels = "+".join(name_of(i) for i in insts)
    return f"{entry}-{kernels}-{H}x{W}-" + (f"in_place+{o}" if in_place else offset_id(insts[0][0], W, o[0]))


E_BIG = (4096, 2052)                                                  # the Y plane: H * W / 16 > 2048 * 256
E_CASES = [("second_sweep_vector_arm", E_BIG, 0), ("byte_arm", (2, 6), 0), ("byte_arm_from_an_odd_base", (64, 128), 1)]

STAGE_ORDER = ("color_lut", "chroma_denoise", "luma_denoise", "local_contrast", "sharpen")   # ISP._finished's
SUBSETS = [tuple(s for s, on in zip(STAGE_ORDER, bits) if on) for bits in itertools.product((0, 1), repeat=5)]
YUV_SUBSETS = [s for s in SUBSETS if "color_lut" not in s]
F_ENTRY = {"color_lut": ("mi_isp_color_lut_rgb_batch", None),
           "chroma_denoise": ("mi_isp_chroma_denoise_rgb_batch", "mi_isp_chroma_denoise_yuv420_batch"),
           "luma_denoise": ("mi_isp_luma_denoise_rgb_batch", "mi_isp_luma_denoise_yuv420_batch"),
           "local_contrast": ("mi_isp_local_contrast_rgb_batch", "mi_isp_local_contrast_yuv420_batch"),
           "sharpen": ("mi_isp_sharpen_rgb_batch", "mi_isp_sharpen_yuv420_batch")}


def b_id(case):
    inst, H, W, path = case
    return f"{name_of(inst)}-{H}x{W}-{path}"


def d_id(case):
    inst, H, W = case
    return f"{name_of(inst)}-{H}x{W}-extremes"


def e_id(case):
    return f"{COPY_KERNEL}-{case[0]}-{case[1][0]}x{case[1][1]}"


def subset_id(s):
    return "+".join(s) or "none"


# ---- inputs and references (made once, read-only, shared by the CPU section and the GPU tests) ---------------------------
def _rng(*key):
    return np.random.default_rng([20262, *[int(k) for k in key]])


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def image_shape(form, H, W):
    return (H, W, 3) if form == "rgb" else (H * 3 // 2, W)


NOISE = 16      # the two noise filters' random bytes: 100 .. 115, so that taps pass and fail their thresholds (6 .. 14) at every size


@functools.lru_cache(maxsize=None)
def random_image(form, H, W, stage=None):
    """Random bytes; for the two noise filters, which leave uniform bytes as they are at the feature tests' thresholds,
    random bytes of NOISE levels."""
    rng = _rng(1, form == "rgb", H, W)
    if stage in ("ydn", "cdn"):
        return _frozen((100 + rng.integers(0, NOISE, image_shape(form, H, W))).astype(np.uint8))
    return _frozen(rng.integers(0, 256, image_shape(form, H, W)).astype(np.uint8))


def seam_tiles(H, W):
    """A local contrast tiling whose tile edges in x cut a 4-pixel group at least once and, where the image has a column
    that could (W >= 8), fall on a multiple of 4 at least once: the first Tx that does, two tile rows where there are two
    rows."""
    for Tx in range(2, min(16, W) + 1):
        edges = R.tile_bounds(W, Tx)[1:-1]
        if any(e % 4 for e in edges) and (W < 8 or any(e % 4 == 0 for e in edges)):
            return (min(2, H), Tx)
    raise AssertionError(f"no tiling for {H}x{W}")


def tilings(inst, H, W):
    return [(1, 1), seam_tiles(H, W)] if inst[0] == "lc" else [None]


def clut_table(cap, kind="random"):
    N = CLUT[cap][0]
    if kind == "random":
        return CL.gpu_tables(N)["random"]
    return _frozen(255 - CL.identity_table(N))                        # black to white, white to black


def reference(inst, img, setting, tiles=None, table="random"):
    """The restatement of the instance's stage on img."""
    stage, form, r = inst
    rgb = form == "rgb"
    if stage == "shp":
        a, t, o = setting
        return (S.sharpen_rgb if rgb else S.sharpen_yuv420)(img, a, r, t, o)
    if stage == "ydn":
        return (Y.luma_denoise_rgb if rgb else Y.luma_denoise_yuv420)(img, r, *setting)
    if stage == "cdn":
        return (C.chroma_denoise_rgb if rgb else C.chroma_denoise_yuv420)(img, r, *setting)
    if stage == "lc":
        return (R.clahe_rgb if rgb else R.clahe_yuv420)(img, tiles, *setting)
    return CL.color_lut_rgb(img, clut_table(r, table), setting)


@functools.lru_cache(maxsize=None)
def b_reference(inst, H, W, k, tiles):
    return _frozen(reference(inst, random_image(inst[1], H, W, inst[0]), SETTINGS[inst[0]][k], tiles))


def settings_of(ti, inst, setting, tiles=None, table="random"):
    stage, _, r = inst
    if stage == "shp":
        return ti.Sharpen(setting[0], r, setting[1], setting[2])
    if stage == "ydn":
        return ti.LumaDenoise(r, *setting)
    if stage == "cdn":
        return ti.ChromaDenoise(r, *setting)
    if stage == "lc":
        return ti.LocalContrast(tiles, *setting)
    return ti.ColorLut(clut_table(r, table), setting)


def run_public(ti, inst, t, s):
    """The instance through the public function (the colour LUT, whose instance only the _path entry point can force,
    through that, into a fresh tensor as the public function would)."""
    stage, form, r = inst
    if stage == "clut":
        out = torch.empty_like(t)
        assert abi(ti, [t], [out], t.shape[0], t.shape[1], s, CLUT[r][1]) == 0
        return out
    mod, fn = {"shp": (ti.sharpen, "unsharp_mask"), "ydn": (ti.luma_denoise, "luma_denoise"),
               "cdn": (ti.chroma_denoise, "chroma_denoise"), "lc": (ti.local_contrast, "clahe")}[stage]
    return getattr(mod, fn + ("" if form == "rgb" else "_yuv420"))(t, s)


# ---- the extremes of D -----------------------------------------------------------------------------------------------------
def dot_sites(H, W):
    """The isolated pixels: the four corners, both sides of the tile seams (column 128, row 64), a thread's first and last
    column (4 g and 4 g + 3) and the two between; at least 4 rows or 4 cells apart, so every window holds one."""
    sites = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (20, TILE_W - 1), (28, TILE_W), (TILE_H - 1, 40), (TILE_H, 48),
             (36, 60), (44, 67), (10, 61), (52, 62)]
    assert 60 % 4 == 0 and 67 % 4 == 3 and H > TILE_H and W > TILE_W
    return sites


DOT_COLOURS = ((255, 255, 255), (255, 0, 0), (0, 255, 255))          # white, then the two whose channels differ most in luma


@functools.lru_cache(maxsize=None)
def extreme_image(stage, form, H, W, kind):
    sites = dot_sites(H, W)
    rr, cc = np.mgrid[0:H, 0:W]
    if stage == "cdn":
        cells = sorted({(r // 2, c // 2) for r, c in sites})
        Hc, Wc = (H + 1) // 2, (W + 1) // 2
        dots = np.zeros((Hc, Wc), bool)
        for a, b in cells:
            dots[a, b] = True
        cr, ccol = np.mgrid[0:Hc, 0:Wc]
        checker = (cr + ccol) % 2 == 1
        if form == "rgb":
            # white cells in a blue field take the largest db a byte at 255 can (SB 0 against 904: inside 4 tc = 1020), black
            # cells in a yellow field the most negative one a byte at 0 can; peak / trough: SB exactly 1020 apart
            green = [g for g in range(256) if int(S.luma(np.array([0, g, 0], np.uint8))) == int(S.luma(np.array([0, 0, 255], np.uint8)))][0]
            on, hi, lo = {"dots": (dots, (255, 255, 255), (0, 0, 255)), "holes": (dots, (0, 0, 0), (255, 255, 0)),
                          "checker": (checker, (255, 255, 255), (0, 0, 255)), "peak": (dots, (0, green, 0), (0, 0, 255)),
                          "trough": (dots, (0, 0, 255), (0, green, 0))}[kind]
            on = np.repeat(np.repeat(on, 2, 0), 2, 1)[:H, :W]
            return _frozen(np.where(on[..., None], np.array(hi, np.uint8), np.array(lo, np.uint8)).astype(np.uint8))
        u = {"dots": dots, "holes": ~dots, "checker": checker}[kind]
        y = ((rr + cc) % 2 * 255).astype(np.uint8)
        uv = np.stack([u, ~u]).astype(np.uint8) * 255
        return _frozen(np.concatenate([y, uv.reshape(H // 2, W)]))
    dots = np.zeros((H, W), bool)
    for r, c in sites:
        dots[r, c] = True
    if form == "yuv":
        y = {"dots": dots * 255, "holes": ~dots * 255, "checker": (rr + cc) % 2 * 255}[kind].astype(np.uint8)
        chroma = _rng(2, H, W).integers(0, 256, (H // 2, W)).astype(np.uint8)
        return _frozen(np.concatenate([y, chroma]))
    if kind == "checker":
        return _frozen(np.repeat(((rr + cc) % 2 * 255).astype(np.uint8)[..., None], 3, 2))
    img = np.zeros((H, W, 3), np.uint8)
    for k, (r, c) in enumerate(sorted(sites)):
        img[r, c] = DOT_COLOURS[k % 3]
    return _frozen(img if kind == "dots" else 255 - img)


def extreme_table(inst):
    return "inverse" if inst[0] == "clut" else "random"


@functools.lru_cache(maxsize=None)
def d_reference(inst, H, W, kind):
    tiles = (1, 1) if inst[0] == "lc" else None
    return _frozen(reference(inst, extreme_image(inst[0], inst[1], H, W, kind), EXTREME[inst[0]], tiles, extreme_table(inst)))


def extreme_deltas(inst, img):
    """(the bytes the deltas are added to, the deltas before the clamp, broadcast to them) of the restatement at EXTREME"""
    stage, form, r = inst
    H, W = (img.shape[0], img.shape[1]) if form == "rgb" else (img.shape[0] * 2 // 3, img.shape[1])
    if stage == "cdn":
        cells = C.cells_rgb(img) if form == "rgb" else C.cells_yuv420(img)
        db, dr, dg = C.deltas(*cells, r, *EXTREME["cdn"])
        if form == "rgb":
            return img.astype(np.int64), np.stack([C._per_pixel(x, H, W) for x in (dr, dg, db)], -1)
        return img[H:].reshape(2, H // 2, W // 2).astype(np.int64), np.stack([db, dr])
    if stage == "clut":
        return img.astype(np.int64), d_reference_of_table(inst, img).astype(np.int64) - img
    L = S.luma(img) if form == "rgb" else img[:H].astype(np.int32)
    if stage == "shp":
        a, t, o = EXTREME["shp"]
        dl = S.delta(L, a, r, t, o)
    elif stage == "ydn":
        dl = Y.delta(L, r, *EXTREME["ydn"])
    else:
        dl = R.delta(L, (1, 1), *EXTREME["lc"])
    dl = np.asarray(dl).astype(np.int64)
    return (img.astype(np.int64), np.repeat(dl[..., None], 3, 2)) if form == "rgb" else (img[:H].astype(np.int64), dl)


def d_reference_of_table(inst, img):
    return CL.color_lut_rgb(img, clut_table(inst[2], "inverse"), 1.0)


def delta_bounds(inst):
    """(the most negative, the most positive) delta the contract of DESIGN.md 3 admits for the instance at EXTREME."""
    stage, form, r = inst
    if stage == "shp":
        # d = S L - Bl with the centre tap b_c^2 L inside Bl: |d| <= (S - b_c^2) 255; delta = (A d + half) >> k, a floor
        b = S.TAPS[r]
        s, A = sum(b) ** 2, S.amount_q6(EXTREME["shp"][0])
        k = 6 + s.bit_length() - 1
        d = (s - b[r] ** 2) * 255
        return (-A * d + (1 << (k - 1))) >> k, (A * d + (1 << (k - 1))) >> k
    if stage == "ydn":
        # m = (2 s + n) // (2 n) over the window, p itself in it: furthest from L(p) with the n - 1 others at the other end
        n = (2 * r + 1) ** 2
        return (2 * 255 + n) // (2 * n) - 255, (2 * 255 * (n - 1) + n) // (2 * n)
    if stage == "lc":
        return -255, 255                                              # E and L are both 0 .. 255, S = 64
    if stage == "clut":
        return -255, 255                                              # y and v are both 0 .. 255, S = 64
    # cdn: db = (2 DB S + 256 n) // (512 n), DB over n - 1 other cells of SB(q) - SB(p); SB is linear in the channels, so its
    # ends are at two of the eight corner colours (RGB), or 4 U (planar)
    n = (2 * r + 1) ** 2
    if form == "rgb":
        corners = np.array(list(itertools.product((0, 255), repeat=3)), np.uint8)
        sb = [int(C.cells_rgb(np.broadcast_to(c, (2, 2, 3)).copy())[1][0, 0]) for c in corners]
        span = min(max(sb) - min(sb), 4 * EXTREME["cdn"][1])             # a tap passes |SB(q) - SB(p)| <= 4 tc
    else:
        span = min(4 * 255, 4 * EXTREME["cdn"][1])
    D = (n - 1) * span
    return (-2 * D * 64 + 256 * n) // (512 * n), (2 * D * 64 + 256 * n) // (512 * n)


def bounded_channel(inst, d):
    """The deltas delta_bounds speaks of: chroma noise reduction's db (B of RGB, U of the planar form)."""
    if inst[0] != "cdn":
        return d
    return d[..., 2] if inst[1] == "rgb" else d[0]


# =========================================================================================================================
# A. no GPU
# =========================================================================================================================
def profile_kernels():
    with open(os.path.join(ROOT, "profiles", "u8_front_end_resources.txt")) as f:
        text = f.read()
    return re.findall(r"^((?:shp|lc|cdn|ydn|clut)::\w+_kernel(?:<[^>]*>)?)\s", text, flags=re.M)


def test_the_instance_table_is_the_cross_product_and_the_profiles_kernels():
    want = ([("shp", f, r) for f in FORMS for r in (1, 2)] + [("ydn", f, r) for f in FORMS for r in (1, 2, 3)]
            + [("cdn", f, r) for f in FORMS for r in (1, 2, 3)] + [("lc", f, None) for f in FORMS]
            + [("clut", "rgb", c) for c in (0, 4913, 35937)])
    assert sorted(map(str, INSTANCES)) == sorted(map(str, want)) and len(set(INSTANCES)) == len(INSTANCES) == 21
    names = {k for i in INSTANCES for k in kernels_of(i)}
    listed = profile_kernels()
    assert len(listed) == len(set(listed)) == 25
    assert names == set(listed)
    assert [4913, 35937] == [17 ** 3, 33 ** 3] and all(CLUT[c][0] ** 3 <= c for c in CLUT if c)
    assert CLUT[0][0] > 33                                             # no LDS instance could take it


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_constants_are_the_sources():
    stage_h = read("isp_u8_stage.h")
    for const, value in (("TILE_W", TILE_W), ("TILE_H", TILE_H), ("MAX_IMAGES", MAX_IMAGES), ("THREADS", THREADS)):
        found = re.findall(rf"constexpr int {const} = (\d+);", stage_h)
        assert found == [str(value)], f"{const} is {found}, the tests assume {value}"
    copy = read("isp_u8_stage.hip")
    assert re.findall(r"blocks > (\d+) \? (\d+) : blocks", copy) == [(str(COPY_BLOCKS),) * 2]
    assert re.findall(r"const size_t blocks = \(count / (\d+) \+ THREADS - 1\) / THREADS;", copy) == [str(COPY_BYTES)]
    assert len(re.findall(r"reinterpret_cast<uint4\*>\(d\)\[i\]", copy)) == 1          # 16 bytes per thread and step
    clut_h = read("isp_color_lut.h")
    for const, value in (("PIXELS_PER_THREAD", CLUT_PIXELS_PER_THREAD), ("LDS_THREADS", CLUT_LDS_THREADS),
                         ("GLOBAL_THREADS", CLUT_GLOBAL_THREADS), ("LDS_POINTS_SMALL", 17), ("LDS_POINTS", 33)):
        found = re.findall(rf"constexpr int {const} = (\d+);", clut_h)
        assert found == [str(value)], f"{const} is {found}, the tests assume {value}"
    assert chunk_of(0) == 1024 and chunk_of(4913) == chunk_of(35937) == 4096
    # the shapes' claims
    for (H, W) in RGB_DWORD + YUV_DWORD:
        assert W % 4 == 0
    for (H, W) in RGB_BYTE + YUV_BYTE + SHP_YUV_BYTE:
        assert W % 4 != 0
    assert all(H % 2 == 0 and W % 2 == 0 for H, W in YUV_DWORD + YUV_BYTE) and all(H % 2 == 0 for H, W in SHP_YUV_BYTE)
    assert (TILE_H, TILE_W) in RGB_DWORD and (TILE_H + 1, TILE_W + 4) in RGB_DWORD and (TILE_H, TILE_W) in YUV_DWORD
    assert min(H for H, W in RGB_DWORD) < 2 * 1 + 1                    # H < 2 R + 1 for every radius
    assert E_BIG[0] * E_BIG[1] > COPY_BLOCKS * THREADS * COPY_BYTES and E_BIG[0] * E_BIG[1] % 16 == 0
    assert E_BIG[0] % 2 == 0 and E_BIG[1] % 2 == 0
    assert (2 * 6) % 16 != 0 and (64 * 128) % 16 == 0                  # the byte arm by its count, and by its base alone


def test_the_settings_are_the_feature_tests():
    assert all(s in SHP_SETTINGS for s in SETTINGS["shp"]) and all(s in YDN_SETTINGS for s in SETTINGS["ydn"])
    assert all(s in CDN_SETTINGS for s in SETTINGS["cdn"])
    assert all(c in LC_CLIPS and s in LC_STRENGTHS for c, s in SETTINGS["lc"])
    assert all(s in CL.GPU_STRENGTHS for s in SETTINGS["clut"])
    assert EXTREME["shp"] in SHP_SETTINGS and EXTREME["ydn"] in YDN_SETTINGS and EXTREME["cdn"] in CDN_SETTINGS


def test_every_kernel_is_named_by_a_case():
    ids = ([b_id(c) for c in B_CASES] + [c_id(c) for c in C_CASES] + [c_id(c, True) for c in C_IN_PLACE]
           + [d_id(c) for c in D_CASES] + [e_id(c) for c in E_CASES])
    assert len(ids) == len(set(ids))
    for section in ([b_id(c) for c in B_CASES], [d_id(c) for c in D_CASES]):
        for kernel in profile_kernels():
            assert any(kernel in i for i in section), kernel
    assert all(COPY_KERNEL in e_id(c) for c in E_CASES)
    entries = {c[0] for c in C_CASES}
    assert entries == set(ALL_ENTRIES) and len(ALL_ENTRIES) == 10
    for kernel in profile_kernels():
        assert any(kernel in c_id(c) for c in C_CASES), kernel


def test_local_contrast_tilings_cut_and_keep_groups():
    shapes = {(H, W) for i, H, W, _ in B_CASES if i[0] == "lc"} | {hw for i in TILE_INSTANCES if i[0] == "lc" for hw in c_shapes(i)}
    for H, W in sorted(shapes):
        Ty, Tx = seam_tiles(H, W)
        assert 1 <= Ty <= H and 2 <= Tx <= min(W, 16)
        edges = R.tile_bounds(W, Tx)[1:-1]
        assert any(e % 4 for e in edges), (H, W)
        if W >= 8:                                                    # (below, the image's own edges are the multiples of 4)
            assert any(e % 4 == 0 for e in edges), (H, W)
    assert seam_tiles(65, 132) == (2, 5)


@pytest.mark.parametrize("inst", INSTANCES, ids=name_of)
def test_no_case_of_b_is_vacuous(inst):
    """Every reference of B differs from its input, and the two settings from one another."""
    for i, H, W, _ in B_CASES:
        if i != inst:
            continue
        img = random_image(inst[1], H, W, inst[0])
        for tiles in tilings(inst, H, W):
            refs = [b_reference(inst, H, W, k, tiles) for k in (0, 1)]
            for k, ref in enumerate(refs):
                assert not np.array_equal(ref, img), f"{H}x{W} setting {k} tiles {tiles}: the input comes back"
            assert not np.array_equal(refs[0], refs[1]), f"{H}x{W} tiles {tiles}: the settings agree"
            if inst[1] == "yuv":                                      # what the planar form leaves alone
                keep = slice(0, H) if inst[0] == "cdn" else slice(H, None)
                assert_exact(refs[0][keep], img[keep], "the untouched plane")


@pytest.mark.parametrize("case", D_CASES, ids=d_id)
def test_the_extremes_reach_the_contracts_bounds(case):
    inst, H, W = case
    lo, hi = delta_bounds(inst)
    assert lo < 0 < hi
    seen_lo, seen_hi, below, above = 0, 0, False, False
    for kind in extreme_kinds(inst):
        img = extreme_image(inst[0], inst[1], H, W, kind)
        if kind not in ("peak", "trough"):
            assert set(np.unique(img[:H] if inst[1] == "yuv" and inst[0] != "cdn" else img)) <= {0, 255}
        base, d = extreme_deltas(inst, img)
        ref = d_reference(inst, H, W, kind)
        if inst[:2] == ("lc", "yuv") and kind == "holes":
            # a white plane with a few black pixels is equalisation's fixed point: the one identity here, on purpose
            assert np.array_equal(ref, img)
        elif inst[0] == "shp" and np.array_equal(ref, img):
            # sharpening pushes 0 and 255 outward: where every channel of a pixel is at its end, every delta saturates
            assert (d != 0).any() and ((base + d <= 0) | (base + d >= 255) | (d == 0)).all()
        else:
            assert not np.array_equal(ref, img), f"{kind}: the input comes back"
        # the restatement's output is its clamped sum: the deltas read here are the ones it adds
        part = ref if inst[1] == "rgb" else (ref[H:].reshape(2, H // 2, W // 2) if inst[0] == "cdn" else ref[:H])
        assert_exact(np.clip(base + d, 0, 255).astype(np.uint8), part, f"{kind}: base + delta")
        b = bounded_channel(inst, d)
        assert lo <= b.min() and b.max() <= hi, f"{kind}: deltas {b.min()} .. {b.max()} outside the contract's {lo} .. {hi}"
        seen_lo, seen_hi = min(seen_lo, int(b.min())), max(seen_hi, int(b.max()))
        below |= bool((base + d < 0).any())
        above |= bool((base + d > 255).any())
    assert seen_hi == hi, f"the largest delta {seen_hi} stays below the contract's {hi}"
    if inst[0] != "lc":
        assert seen_lo == lo, f"the most negative delta {seen_lo} stays above the contract's {lo}"
    elif inst[1] == "rgb":                                            # E(255) == 255: -255 cannot occur; the cyan dot falls
        assert seen_lo <= -128
    else:                                                             # a plane of 0 and 255 alone: equalisation only lifts
        assert seen_lo == 0
    if inst[:2] in CLAMPING:
        assert below and above, "no byte saturates at 0 and at 255"
    else:
        assert not below and not above                                # the contract's own: nothing to clamp
    if inst[0] == "shp":
        assert hi >= 6 * 255 and lo <= -6 * 255                        # pair()'s 16-bit lanes, far past a byte


# =========================================================================================================================
# the GPU tests
# =========================================================================================================================
@pytest.fixture(scope="module")
def ti():
    import taichi_image_amd as t
    return t


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def to_dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                      # (a copy: the shared inputs are read-only)


# ---- B --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", B_CASES, ids=b_id)
def test_every_instance_at_the_seams_of_the_dword_path(ti, dev, case):
    inst, H, W, path = case
    img = random_image(inst[1], H, W, inst[0])
    t = to_dev(img, dev)
    assert t.data_ptr() % 16 == 0 and (W % 4 == 0) == (path == "dword")
    for tiles in tilings(inst, H, W):
        for k, setting in enumerate(SETTINGS[inst[0]]):
            got = run_public(ti, inst, t, settings_of(ti, inst, setting, tiles))
            assert got.data_ptr() % 16 == 0 and got.data_ptr() != t.data_ptr()
            got = got.cpu().numpy()
            ref = b_reference(inst, H, W, k, tiles)
            what = f"{b_id(case)} setting {setting} tiles {tiles}"
            assert_exact(got, ref, what)
            if inst[1] == "yuv":
                keep = slice(0, H) if inst[0] == "cdn" else slice(H, None)
                assert_exact(got[keep], img[keep], what + ": the untouched plane")
    assert_exact(t.cpu().numpy(), img, "the input is left alone")


# ---- C --------------------------------------------------------------------------------------------------------------------
PAD = 64


def call_at(entry, img, H, W, args, dev, src_off, dst_off, in_place=False):
    """One image through the entry point `entry` (src, dst, 1, H, W, *args, stream), source and destination src_off and
    dst_off bytes past a 16-byte boundary inside buffers of SENTINEL bytes (in place: one buffer).  Returns the output
    after asserting that the bytes before and behind each image, and a source filtered into another buffer, came back as
    they went in."""
    from taichi_image_amd import _native
    size = img.size

    def buffer():
        b = torch.full((PAD + size + PAD,), SENTINEL, dtype=torch.uint8, device=dev)
        assert b.data_ptr() % 16 == 0
        return b
    sbuf, s0 = buffer(), PAD + src_off
    sbuf[s0:s0 + size] = torch.from_numpy(np.array(img).ravel()).to(dev)
    dbuf, d0 = (sbuf, s0) if in_place else (buffer(), PAD + dst_off)
    sp, dp = sbuf.data_ptr() + s0, dbuf.data_ptr() + d0
    assert sp % 4 == src_off % 4 and dp % 4 == (src_off if in_place else dst_off) % 4
    rc = getattr(_native.lib(), entry)((ctypes.c_void_p * 1)(sp), (ctypes.c_void_p * 1)(dp), 1, H, W, *args,
                                       _native.stream_ptr(dev))
    _native.check(rc)
    s, d = sbuf.cpu().numpy(), dbuf.cpu().numpy()
    assert (d[:d0] == SENTINEL).all() and (d[d0 + size:] == SENTINEL).all(), "bytes around the destination were written"
    if not in_place:
        assert (s[:s0] == SENTINEL).all() and (s[s0 + size:] == SENTINEL).all(), "bytes around the source were written"
        assert np.array_equal(s[s0:s0 + size], np.asarray(img).ravel()), "the source was written"
    return d[d0:d0 + size].reshape(img.shape).copy()


def abi_args(ti, inst, entry, s, n, dev):
    """(the arguments between the shape and the stream, what must stay alive until the call returns)"""
    from taichi_image_amd import _native
    if inst[0] == "lc":
        ws = torch.empty(int(_native.lib().mi_isp_local_contrast_workspace_bytes(n, s._arg())), dtype=torch.uint8, device=dev)
        return (s._arg(), ws.data_ptr()), ws
    if inst[0] == "clut":
        table = s._device_table(dev)
        return (table.data_ptr(), s._arg()) + ((CLUT[inst[2]][1],) if entry == CLUT_PATH_ENTRY else ()), table
    return (s._arg(),), None


def c_case(ti, dev, insts, k):
    """(instance, image, H, W, the settings, the reference) per instance of a C case"""
    for inst in insts:
        H, W = c_shapes(inst)[k]
        img = random_image(inst[1], H, W, inst[0])
        tiles = seam_tiles(H, W) if inst[0] == "lc" else None
        setting = SETTINGS[inst[0]][0]
        ref = reference(inst, img, setting, tiles)
        assert not np.array_equal(ref, img)
        yield inst, img, H, W, settings_of(ti, inst, setting, tiles), ref


@gpu
@pytest.mark.parametrize("case", C_CASES, ids=c_id)
def test_the_alignment_fork_through_the_c_abi(ti, dev, case):
    entry, insts, k, (oname, src_off, dst_off) = case
    for inst, img, H, W, s, ref in c_case(ti, dev, insts, k):
        args, alive = abi_args(ti, inst, entry, s, 1, dev)
        aligned = call_at(entry, img, H, W, args, dev, 0, 0)
        got = call_at(entry, img, H, W, args, dev, src_off, dst_off)
        what = f"{entry} {name_of(inst)} {H}x{W} {oname}"
        assert_exact(aligned, ref, what + ": the aligned call")
        assert_exact(got, aligned, what + " against the aligned call")
        assert_exact(got, ref, what)


@gpu
@pytest.mark.parametrize("case", C_IN_PLACE, ids=lambda c: c_id(c, True))
def test_in_place_at_an_even_and_an_odd_base(ti, dev, case):
    """dst[i] == src[i] exactly is the one overlap the front end takes: it still gives the reference."""
    entry, insts, k, off = case
    for inst, img, H, W, s, ref in c_case(ti, dev, insts, k):
        args, alive = abi_args(ti, inst, entry, s, 1, dev)
        got = call_at(entry, img, H, W, args, dev, off, off, in_place=True)
        assert_exact(got, ref, f"{entry} {name_of(inst)} {H}x{W} in place at +{off}")


# ---- D --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", D_CASES, ids=d_id)
def test_the_write_back_at_its_bounds(ti, dev, case):
    inst, H, W = case
    tiles = (1, 1) if inst[0] == "lc" else None
    s = settings_of(ti, inst, EXTREME[inst[0]], tiles, extreme_table(inst))
    for kind in extreme_kinds(inst):
        img = extreme_image(inst[0], inst[1], H, W, kind)
        got = run_public(ti, inst, to_dev(img, dev), s).cpu().numpy()
        assert_exact(got, d_reference(inst, H, W, kind), f"{d_id(case)} {kind}")


# ---- E --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", E_CASES, ids=e_id)
def test_the_plane_copy(ti, dev, case):
    """Chroma noise reduction at strength 0 is an identity whose Y plane is the plane copy's."""
    _, (H, W), off = case
    n = H * W * 3 // 2
    g = torch.Generator(device=dev)
    g.manual_seed(20262)
    buf = torch.randint(0, 256, (n + 16,), dtype=torch.uint8, device=dev, generator=g)
    yuv = buf[off:off + n].view(H * 3 // 2, W)
    assert yuv.data_ptr() % 16 == off and yuv.is_contiguous()
    before = yuv.clone()
    out = ti.chroma_denoise.chroma_denoise_yuv420(yuv, ti.ChromaDenoise(1, 255, 255, 0.0))
    assert out.data_ptr() != yuv.data_ptr() and out.data_ptr() % 16 == 0
    assert torch.equal(out, before), "the copy is not the input"
    assert torch.equal(yuv, before), "the input was written"
    assert int(before[:H].max()) > int(before[:H].min())


# ---- F --------------------------------------------------------------------------------------------------------------------
def stage_settings(ti):
    return dict(color_lut=ti.ColorLut(CL.gpu_tables(LUT_N)["look"], LUT_STRENGTH), chroma_denoise=ti.ChromaDenoise(*CDN_ARGS),
                luma_denoise=ti.LumaDenoise(*LDN_ARGS), local_contrast=ti.LocalContrast(*LC_ARGS), sharpen=ti.Sharpen(*SHARP_ARGS))


def compose(x, subset, yuv, what):
    """The references in ISP._finished's order; every stage of the subset must move the image."""
    step = {"color_lut": lambda v: CL.color_lut_rgb(v, CL.gpu_tables(LUT_N)["look"], LUT_STRENGTH),
            "chroma_denoise": lambda v: (C.chroma_denoise_yuv420 if yuv else C.chroma_denoise_rgb)(v, *CDN_ARGS),
            "luma_denoise": lambda v: (Y.luma_denoise_yuv420 if yuv else Y.luma_denoise_rgb)(v, *LDN_ARGS),
            "local_contrast": lambda v: (R.clahe_yuv420 if yuv else R.clahe_rgb)(v, *LC_ARGS),
            "sharpen": lambda v: (S.sharpen_yuv420 if yuv else S.sharpen_rgb)(v, *SHARP_ARGS)}
    for name in STAGE_ORDER:
        if name in subset:
            y = step[name](x)
            assert not np.array_equal(y, x), f"{what}: {name} leaves its input as it is"
            x = y
    return x


def counters(monkeypatch):
    return {name: _count_calls(monkeypatch, name) for name in ALL_ENTRIES}


def check_counts(counts, subset, yuv, calls=1):
    want = {name: 0 for name in ALL_ENTRIES}
    for s in subset:
        want[F_ENTRY[s][1 if yuv else 0]] = calls
    assert {k: len(v) for k, v in counts.items()} == want


def tonemap(isp, frames, yuv):
    imgs = isp.load_packed12_batch(frames)
    fn = isp.tonemap_reinhard_yuv420 if yuv else isp.tonemap_reinhard
    return [o.cpu().numpy() for o in fn(imgs, gamma=0.7)]


def isp_subset(ti, rng, dev, monkeypatch, cam, subset, H, W, yuv):
    frames = frames_of(rng, dev, H, W, 2)
    kw = dict(moving_alpha=0.3, device=dev)
    all_settings = stage_settings(ti)
    plain = getattr(ti, cam)(ti.BayerPattern.RGGB, **kw)
    isp = getattr(ti, cam)(ti.BayerPattern.RGGB, **{s: all_settings[s] for s in subset}, **kw)
    want = tonemap(plain, frames, yuv)
    counts = counters(monkeypatch)
    got = tonemap(isp, frames, yuv)
    check_counts(counts, subset, yuv)
    for k, (g, w) in enumerate(zip(got, want)):
        what = f"{cam} {'yuv420 ' if yuv else ''}{subset_id(subset)} output {k}"
        assert_exact(g, compose(w, subset, yuv, what), what)
    assert_exact(isp.metrics.cpu().numpy(), plain.metrics.cpu().numpy(), "the metering state")


@gpu
@pytest.mark.parametrize("subset", SUBSETS, ids=subset_id)
def test_every_subset_of_the_stages_through_the_isp(ti, rng, dev, monkeypatch, subset):
    isp_subset(ti, rng, dev, monkeypatch, "Camera16", subset, 66, 100, False)


@gpu
@pytest.mark.parametrize("subset", YUV_SUBSETS, ids=subset_id)
def test_every_subset_of_the_planar_stages_through_the_isp(ti, rng, dev, monkeypatch, subset):
    isp_subset(ti, rng, dev, monkeypatch, "Camera16", subset, 64, 96, True)


@gpu
def test_the_full_set_on_camera32(ti, rng, dev, monkeypatch):
    isp_subset(ti, rng, dev, monkeypatch, "Camera32", STAGE_ORDER, 66, 100, False)


@gpu
def test_a_walk_through_set(ti, rng, dev, monkeypatch):
    """Each stage turned on in an order that is not the order of application, two turned off again: after every step the
    outputs are the references of the stages that are on, composed in _finished's order, and only those are launched."""
    H, W = 66, 100
    frames = frames_of(rng, dev, H, W, 1)
    kw = dict(moving_alpha=0.3, device=dev)
    plain, isp = ti.Camera16(ti.BayerPattern.RGGB, **kw), ti.Camera16(ti.BayerPattern.RGGB, **kw)
    settings = stage_settings(ti)
    on = set()
    walk = [("sharpen", True), ("color_lut", True), ("luma_denoise", True), ("local_contrast", True), ("chroma_denoise", True),
            ("luma_denoise", False), ("color_lut", False)]
    assert [s for s, _ in walk[:5]] != list(STAGE_ORDER) and sorted(s for s, _ in walk[:5]) == sorted(STAGE_ORDER)
    counts = counters(monkeypatch)
    for step, (name, turn_on) in enumerate([(None, None)] + walk):
        if name is not None:
            isp.set(**{name: settings[name] if turn_on else False})
            (on.add if turn_on else on.discard)(name)
        subset = tuple(s for s in STAGE_ORDER if s in on)
        assert {s for s in STAGE_ORDER if getattr(isp, s) is not None} == on
        for c in counts.values():
            c.clear()
        want = tonemap(plain, frames, False)
        got = tonemap(isp, frames, False)
        check_counts(counts, subset, False)
        what = f"step {step}: {subset_id(subset)}"
        assert_exact(got[0], compose(want[0], subset, False, what), what)


# ---- G --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("entry", ALL_ENTRIES, ids=ALL_ENTRIES)
def test_overlapping_images_are_refused_without_a_launch(ti, dev, entry):
    """A destination one pixel into its own source, and a destination that is the other image's source: status 1, the text
    of the overlap rule, and every byte where it was."""
    from taichi_image_amd import _native
    L = _native.lib()
    (stage, form), = [k for k, v in ENTRY.items() if v == entry] or [("clut", "rgb")]
    inst = [i for i in INSTANCES if i[:2] == (stage, form)][0]
    H, W = 8, 12
    img = random_image(form, H, W, stage)
    size, pixel = img.size, 3 if form == "rgb" else 1
    s = settings_of(ti, inst, SETTINGS[stage][0], (2, 3) if stage == "lc" else None)
    args, alive = abi_args(ti, inst, entry, s, 2, dev)
    src = torch.from_numpy(np.concatenate([img.ravel(), img.ravel()[::-1], np.full(64, 7, np.uint8)])).to(dev)
    before = src.clone()
    dst = torch.full((size + 64,), 99, dtype=torch.uint8, device=dev)
    a, b, d = src.data_ptr(), src.data_ptr() + size, dst.data_ptr()
    stream = _native.stream_ptr(dev)
    ptrs = lambda *p: (ctypes.c_void_p * len(p))(*p)                 # noqa: E731
    fn = getattr(L, entry)
    noun = {"shp": "sharpen", "lc": "local_contrast", "cdn": "chroma_denoise", "ydn": "luma_denoise", "clut": "color_lut"}[stage]
    who = entry[len("mi_isp_"):]
    assert fn(ptrs(a), ptrs(a + pixel), 1, H, W, *args, stream) == 1
    assert L.mi_isp_last_error() == f"{who}: {noun} output 0 overlaps input 0".encode()
    assert fn(ptrs(a + W * pixel), ptrs(a), 1, H, W, *args, stream) == 1
    assert L.mi_isp_last_error() == f"{who}: {noun} output 0 overlaps input 0".encode()
    assert fn(ptrs(a, b), ptrs(d, a), 2, H, W, *args, stream) == 1
    assert L.mi_isp_last_error() == f"{who}: {noun} output 1 overlaps input 0".encode()
    assert fn(ptrs(a, b), ptrs(d, d), 2, H, W, *args, stream) == 1
    assert L.mi_isp_last_error() == f"{who}: {noun} outputs 0 and 1 overlap".encode()
    torch.cuda.synchronize(dev)
    assert torch.equal(src, before) and bool((dst == 99).all())
    # images that touch but do not overlap are taken: the second source ends where the first destination begins
    adjacent = torch.full((3 * size + 64,), 99, dtype=torch.uint8, device=dev)
    adjacent[size:2 * size] = torch.from_numpy(np.array(img).ravel()).to(dev)
    p = adjacent.data_ptr()
    assert fn(ptrs(p + size), ptrs(p + 2 * size), 1, H, W, *args, stream) == 0
    got = adjacent.cpu().numpy()
    tiles = (2, 3) if stage == "lc" else None
    assert_exact(got[2 * size:3 * size].reshape(img.shape), reference(inst, img, SETTINGS[stage][0], tiles), "the adjacent call")
    assert (got[:size] == 99).all() and (got[3 * size:] == 99).all() and np.array_equal(got[size:2 * size], img.ravel())
