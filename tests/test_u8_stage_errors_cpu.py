"""The u8 output stages' host checks without a GPU: each of the ten batch entry points (sharpening, local contrast, chroma and
luma noise reduction in their RGB and YUV 4:2:0 forms, the colour LUT with and without a forced path) rejects a bad argument,
or returns for nothing to do, before any launch, with its return code and its full error text.  The addresses are made up
(host buffers): nothing is launched or dereferenced.  Where the five stages differ is their behaviour and is pinned here:
the least n, the evenness rule of the YUV form, in place, the size limit and the order of the checks (the cases with two
faults: the text says which check came first).  The overlap rule is one for all five: a written image overlaps no read image
and no other written image of the call, dst[i] == src[i] exactly excepted for the stages that run in place."""
import ctypes

import pytest

from taichi_image_amd import _native

H, W = 4, 8
_bufs = [(ctypes.c_uint8 * 4096)() for _ in range(5)]       # disjoint images, each larger than any 4 x 8 one; 16-byte aligned
_A, _B, _C, _D, _WS = [(ctypes.addressof(b) + 15) & ~15 for b in _bufs]


def _ptrs(addresses):
    return None if addresses is None else (ctypes.c_void_p * len(addresses))(*addresses)


def _ref(s):
    return None if s is None else ctypes.byref(s)


def _stencil(name, form):
    def call(L, a):
        return getattr(L, f"mi_isp_{name}_{form}_batch")(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], _ref(a["s"]),
                                                         None)
    return call


def _local_contrast(form):
    def call(L, a):
        return getattr(L, f"mi_isp_local_contrast_{form}_batch")(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"],
                                                                 _ref(a["s"]), a["ws"], None)
    return call


def _color_lut(L, a):
    return L.mi_isp_color_lut_rgb_batch(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], a["table"], _ref(a["s"]), None)


def _color_lut_path(L, a):
    return L.mi_isp_color_lut_rgb_batch_path(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], a["table"], _ref(a["s"]),
                                             a["path"], None)


GOOD = dict(src=[_A], dst=[_B], n=1, H=H, W=W, ws=_WS, table=_C, path=0)
BIG = 1 << 22                                                # rows: past every stage's limit


def _common(noun, few):
    """(case, the bad arguments, the text after "<who>: " or None for a return of 0) that all five stages share; few: the
    text for n below the stage's least"""
    return [
        ("null_settings", dict(s=None), f"null {noun} settings"),
        ("negative_n", dict(n=-1), few(-1)),
        ("bad_shape", dict(H=-1), f"bad {noun} shape -1x{W}"),
        ("null_list", dict(src=None), f"null {noun} image list"),
        ("null_dst_list", dict(dst=None), f"null {noun} image list"),
        ("null_image", dict(src=[0]), f"{noun} image 0 has a null pointer"),
        ("null_second_dst", dict(n=2, src=[_A, _C], dst=[_B, 0]), f"{noun} image 1 has a null pointer"),
        ("settings_before_n", dict(n=-1, s=None), f"null {noun} settings"),
        ("n_before_shape", dict(n=-1, H=-1), few(-1)),
    ]


def _tiled(noun, yuv, sides):
    """the three stages that take one block per 128 x 64 pixels and cannot run in place; sides: the YUV form wants both even"""
    cases = [
        ("too_many_rows", dict(H=BIG), f"{noun} image {BIG}x{W} too large"),
        ("too_many_columns", dict(W=1 << 24), f"{noun} image {H}x{1 << 24} too large"),
        ("too_many_tiles", dict(H=1 << 21, W=1 << 20), f"{noun} image {1 << 21}x{1 << 20} too large"),
        ("in_place", dict(dst=[_A]), f"{noun} image 0: the filter cannot run in place"),
        ("in_place_before_next_null", dict(n=2, src=[_A, 0], dst=[_A, _B]), f"{noun} image 0: the filter cannot run in place"),
        ("list_before_empty", dict(src=None, H=0), f"null {noun} image list"),
        ("size_before_list", dict(src=None, H=BIG), f"{noun} image {BIG}x{W} too large"),
        ("empty_image", dict(H=0, src=[0]), None),
        ("empty_row", dict(W=0, src=[0]), None),
    ]
    if yuv:
        even = ((lambda h, w: f"the Y plane of a {noun} YUV 4:2:0 image must have even sides, got {h}x{w}") if sides else
                (lambda h, w: f"the Y plane of a {noun} YUV 4:2:0 image must have an even height, got {h}"))
        cases += [
            ("odd_height", dict(H=5), even(5, W)),
            # an odd width passes sharpening's rule, so its next fault speaks
            ("odd_width_null_list", dict(W=7, src=None), even(H, 7) if sides else f"null {noun} image list"),
            ("evenness_before_list", dict(H=5, src=None), even(5, W)),
            ("size_before_evenness", dict(H=BIG + 1), f"{noun} image {BIG + 1}x{W} too large"),
        ]
    else:
        cases += [("odd_sides_empty", dict(H=0, W=7, src=[0]), None)]
    return cases


def _overlap(noun, yuv, in_place=False):
    """the overlap checks, every stage's since they became one rule (they were luma noise reduction's alone): a written image
    overlaps no read image and no other written image; in_place: the stage takes dst[i] == src[i] exactly, and only that"""
    size = H * W * 3 // (2 if yuv else 1)                    # bytes of one image
    pixel = 1 if yuv else 3
    cases = [
        ("output_in_input", dict(dst=[_A + size - 1]), f"{noun} output 0 overlaps input 0"),
        ("input_in_output", dict(dst=[_A - size + 1 + 2048], src=[_A + 2048]), f"{noun} output 0 overlaps input 0"),
        ("output_in_other_input", dict(n=2, src=[_A, _C], dst=[_B, _A + 8]), f"{noun} output 1 overlaps input 0"),
        ("outputs_overlap", dict(n=2, src=[_A, _C], dst=[_B, _B + size - 1]), f"{noun} outputs 0 and 1 overlap"),
        ("same_output_twice", dict(n=2, src=[_A, _C], dst=[_B, _B]), f"{noun} outputs 0 and 1 overlap"),
        ("pointers_before_overlap", dict(n=2, src=[_A, 0], dst=[_A + 8, _B]), f"{noun} image 1 has a null pointer"),
    ]
    if in_place:
        cases += [
            # exact in place passes to the next check: image 1's fault speaks, not image 0's
            ("in_place_then_overlap", dict(n=2, src=[_A, _C], dst=[_A, _C + pixel]), f"{noun} output 1 overlaps input 1"),
            ("in_place_shifted_by_a_pixel", dict(dst=[_A + pixel]), f"{noun} output 0 overlaps input 0"),
            ("in_place_shifted_back_by_a_row", dict(src=[_A + W * pixel], dst=[_A]), f"{noun} output 0 overlaps input 0"),
            ("output_is_other_input", dict(n=2, src=[_A, _C], dst=[_B, _A]), f"{noun} output 1 overlaps input 0"),
            ("in_place_output_is_other_input", dict(n=2, src=[_A, _A], dst=[_A, _B]), f"{noun} output 0 overlaps input 1"),
            ("same_image_twice_in_place", dict(n=2, src=[_A, _A], dst=[_A, _A]), f"{noun} output 0 overlaps input 1"),
            ("same_output_twice_one_in_place", dict(n=2, src=[_A, _C], dst=[_A, _A]), f"{noun} outputs 0 and 1 overlap"),
        ]
    return cases


def _sharpen_cases(yuv):
    noun = "sharpen"
    few = lambda n: f"sharpen needs at least one image, got {n}"
    good = _native.Sharpen(64, 1, 0, -1)
    return good, _common(noun, few) + _tiled(noun, yuv, sides=False) + _overlap(noun, yuv) + [
        ("no_image", dict(n=0), few(0)),
        ("no_image_null_list", dict(n=0, src=None), few(0)),
        ("radius", dict(s=_native.Sharpen(64, 3, 0, -1)), "sharpen radius 3 (1 or 2)"),
        ("amount", dict(s=_native.Sharpen(513, 1, 0, -1)), "sharpen amount_q6 513 outside 0 .. 512"),
        ("threshold", dict(s=_native.Sharpen(64, 1, 256, -1)), "sharpen threshold 256 outside 0 .. 255"),
        ("overshoot", dict(s=_native.Sharpen(64, 1, 0, -2)), "sharpen overshoot -2 outside 0 .. 255 (-1: none)"),
        ("settings_before_n", dict(n=0, s=_native.Sharpen(64, 3, 0, -1)), "sharpen radius 3 (1 or 2)"),
    ]


def _chroma_cases(yuv):
    noun = "chroma_denoise"
    good = _native.ChromaDenoise(2, 8, 12, 64)
    return good, _common(noun, lambda n: f"{noun} with {n} images") + _tiled(noun, yuv, sides=True) + _overlap(noun, yuv) + [
        ("no_image", dict(n=0, src=[0]), None),
        ("list_before_no_image", dict(n=0, src=None), f"null {noun} image list"),
        ("radius", dict(s=_native.ChromaDenoise(4, 8, 12, 64)), f"{noun} radius 4 (1, 2 or 3)"),
        ("luma_threshold", dict(s=_native.ChromaDenoise(2, 256, 12, 64)), f"{noun} luma_threshold 256 outside 0 .. 255"),
        ("chroma_threshold", dict(s=_native.ChromaDenoise(2, 8, -1, 64)), f"{noun} chroma_threshold -1 outside 0 .. 255"),
        ("strength", dict(s=_native.ChromaDenoise(2, 8, 12, 65)), f"{noun} strength_q6 65 outside 0 .. 64"),
    ]


def _luma_cases(yuv):
    noun = "luma_denoise"
    good = _native.LumaDenoise(2, 6, 6, 64)
    return good, _common(noun, lambda n: f"{noun} with {n} images") + _tiled(noun, yuv, sides=True) + _overlap(noun, yuv) + [
        ("no_image", dict(n=0, src=[0]), None),
        ("list_before_no_image", dict(n=0, src=None), f"null {noun} image list"),
        ("radius", dict(s=_native.LumaDenoise(0, 6, 6, 64)), f"{noun} radius 0 (1, 2 or 3)"),
        ("threshold", dict(s=_native.LumaDenoise(2, 256, 6, 64)), f"{noun} threshold 256 outside 0 .. 255"),
        ("threshold_bright", dict(s=_native.LumaDenoise(2, 6, -1, 64)), f"{noun} threshold_bright -1 outside 0 .. 255"),
        ("strength", dict(s=_native.LumaDenoise(2, 6, 6, -1)), f"{noun} strength_q6 -1 outside 0 .. 64"),
    ]


def _local_contrast_cases(yuv):
    noun = "local_contrast"
    good = _native.LocalContrast(2, 2, 512, 64)
    cases = _common(noun, lambda n: f"{noun} with {n} images") + _overlap(noun, yuv, in_place=True) + [
        ("tiles", dict(s=_native.LocalContrast(17, 2, 512, 64)), f"{noun} tiles 17 x 2 outside 1 .. 16"),
        ("clip", dict(s=_native.LocalContrast(2, 2, 255, 64)), f"{noun} clip_q8 255 outside 256 .. 16384 (0: no clip)"),
        ("strength", dict(s=_native.LocalContrast(2, 2, 512, 65)), f"{noun} strength_q6 65 outside 0 .. 64"),
        ("tile_fit", dict(s=_native.LocalContrast(8, 8, 512, 64)), f"{noun} image {H}x{W} smaller than its 8 x 8 tiles"),
        ("too_many_rows", dict(H=32770), f"{noun} image 32770x{W} larger than 32768"),
        ("too_many_columns", dict(W=BIG), f"{noun} image {H}x{BIG} larger than 32768"),
        ("null_workspace", dict(ws=None), f"{noun} workspace null or not 16-byte aligned"),
        ("workspace_alignment", dict(ws=_WS + 8), f"{noun} workspace null or not 16-byte aligned"),
        # in place is this stage's to run: the next image's fault speaks
        ("in_place_allowed", dict(n=2, src=[_A, 0], dst=[_A, _B]), f"{noun} image 1 has a null pointer"),
        # nothing to do returns before the list, the tile fit and the workspace are looked at
        ("no_image", dict(n=0, src=None, ws=None, s=_native.LocalContrast(8, 8, 512, 64)), None),
        ("empty_image", dict(H=0, src=None, ws=None, s=_native.LocalContrast(8, 8, 512, 64)), None),
        ("empty_row", dict(W=0, dst=None), None),
        ("tile_fit_before_side", dict(H=32770, W=4, s=_native.LocalContrast(8, 8, 512, 64)),
         f"{noun} image 32770x4 smaller than its 8 x 8 tiles"),
        ("side_before_list", dict(H=32770, src=None), f"{noun} image 32770x{W} larger than 32768"),
        ("list_before_workspace", dict(src=None, ws=None), f"null {noun} image list"),
        ("workspace_before_pointers", dict(ws=None, src=[0]), f"{noun} workspace null or not 16-byte aligned"),
    ]
    if yuv:
        even = lambda h, w: f"the Y plane of a {noun} YUV 4:2:0 image must have even sides, got {h}x{w}"
        cases += [
            ("odd_height", dict(H=5), even(5, W)),
            ("odd_width_null_list", dict(W=7, src=None), even(H, 7)),
            ("evenness_before_no_image", dict(n=0, H=5), even(5, W)),
            ("evenness_before_side", dict(H=32771), even(32771, W)),
        ]
    else:
        cases += [("odd_sides_empty", dict(H=0, W=7, src=None), None)]
    return good, cases


def _color_lut_cases(forced):
    noun = "color_lut"
    good = _native.ColorLut(17, 64)
    cases = _common(noun, lambda n: f"{noun} with {n} images") + _overlap(noun, False, in_place=True) + [
        ("n_points", dict(s=_native.ColorLut(66, 64)), f"{noun} n_points 66 outside 2 .. 65"),
        ("strength", dict(s=_native.ColorLut(17, 65)), f"{noun} strength_q6 65 outside 0 .. 64"),
        ("too_many_pixels", dict(H=1 << 16, W=1 << 15), f"{noun} image {1 << 16}x{1 << 15} too large"),
        ("null_table", dict(table=None), f"null {noun} table"),
        ("table_before_list", dict(table=None, src=None), f"null {noun} table"),
        ("size_before_table", dict(H=1 << 16, W=1 << 15, table=None), f"{noun} image {1 << 16}x{1 << 15} too large"),
        ("list_before_no_image", dict(n=0, src=None), f"null {noun} image list"),
        ("list_before_empty", dict(H=0, src=None), f"null {noun} image list"),
        ("table_before_empty", dict(H=0, table=None), f"null {noun} table"),
        ("no_image", dict(n=0, src=[0]), None),
        ("empty_image", dict(H=0, src=[0]), None),
        # in place is this stage's to run: the next image's fault speaks
        ("in_place_allowed", dict(n=2, src=[_A, 0], dst=[_A, _B]), f"{noun} image 1 has a null pointer"),
    ]
    if forced:
        path = lambda p: f"{noun} path {p} (0: the dispatcher's, 1: LDS, n_points <= 33, 2: global)"
        cases += [
            ("path", dict(path=3), path(3)),
            ("negative_path", dict(path=-1), path(-1)),
            ("lds_path_large_table", dict(path=1, s=_native.ColorLut(34, 64)), path(1)),
            ("path_before_n", dict(path=3, n=-1), path(3)),
            ("strength_before_path", dict(path=3, s=_native.ColorLut(17, 65)), f"{noun} strength_q6 65 outside 0 .. 64"),
        ]
    return good, cases


# who: (entry, (the good settings, the cases))
ENTRIES = {
    "sharpen_rgb_batch": (_stencil("sharpen", "rgb"), _sharpen_cases(False)),
    "sharpen_yuv420_batch": (_stencil("sharpen", "yuv420"), _sharpen_cases(True)),
    "local_contrast_rgb_batch": (_local_contrast("rgb"), _local_contrast_cases(False)),
    "local_contrast_yuv420_batch": (_local_contrast("yuv420"), _local_contrast_cases(True)),
    "chroma_denoise_rgb_batch": (_stencil("chroma_denoise", "rgb"), _chroma_cases(False)),
    "chroma_denoise_yuv420_batch": (_stencil("chroma_denoise", "yuv420"), _chroma_cases(True)),
    "luma_denoise_rgb_batch": (_stencil("luma_denoise", "rgb"), _luma_cases(False)),
    "luma_denoise_yuv420_batch": (_stencil("luma_denoise", "yuv420"), _luma_cases(True)),
    "color_lut_rgb_batch": (_color_lut, _color_lut_cases(False)),
    "color_lut_rgb_batch_path": (_color_lut_path, _color_lut_cases(True)),
}


def _table(who):
    """case -> (bad arguments, text); a later case of one name replaces the earlier (a stage's own form of a shared case)"""
    return {name: (bad, text) for name, bad, text in ENTRIES[who][1][1]}


CASES = [(who, name) for who in ENTRIES for name in _table(who)]


@pytest.mark.parametrize("who,case", CASES, ids=[f"{w}-{c}" for w, c in CASES])
def test_u8_batch_entry_checks_on_the_host(who, case):
    L = _native.lib()
    entry, (good, _) = ENTRIES[who]
    bad, text = _table(who)[case]
    rc = entry(L, {**GOOD, "s": good, **bad})
    if text is None:
        assert rc == 0
    else:
        assert rc == 1
        assert L.mi_isp_last_error() == f"{who}: {text}".encode()


def test_every_entry_point_has_its_cases():
    assert len(ENTRIES) == 10
    n = {who: len(_table(who)) for who in ENTRIES}
    # the YUV forms add the evenness cases; the forced path adds the path cases; every stage has the six overlap cases and
    # the stages that run in place seven more
    assert n == {"sharpen_rgb_batch": 31, "sharpen_yuv420_batch": 34, "local_contrast_rgb_batch": 39,
                 "local_contrast_yuv420_batch": 42, "chroma_denoise_rgb_batch": 31, "chroma_denoise_yuv420_batch": 34,
                 "luma_denoise_rgb_batch": 31, "luma_denoise_yuv420_batch": 34, "color_lut_rgb_batch": 34,
                 "color_lut_rgb_batch_path": 39}
    for who in ENTRIES:
        names = set(_table(who))
        assert {"output_in_input", "input_in_output", "output_in_other_input", "outputs_overlap", "same_output_twice",
                "pointers_before_overlap"} <= names, who
        assert ("in_place_shifted_by_a_pixel" in names) == ("in_place_allowed" in names), who
