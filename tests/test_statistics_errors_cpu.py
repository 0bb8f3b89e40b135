"""The frame statistics' host checks without a GPU: each entry point rejects one bad argument at a time before any launch,
with its return code and its full error text.  The addresses are made up (host buffers): nothing is launched or
dereferenced.  The shared checks word their errors as the raw stages' do (tests/test_raw_stage_errors_cpu.py)."""
import ctypes

import pytest

from taichi_image_amd import _native
from taichi_image_amd._native import MI_F16, MI_F32, MI_RAW_16U, MI_RAW_32F, MI_RAW_PACKED12, MI_RAW_PACKED16, MI_U8

H, W = 4, 8
_bufs = [(ctypes.c_uint64 * 4096)() for _ in range(3)]      # 8-byte aligned planes, each larger than any frame or result here
_addr = [ctypes.addressof(b) for b in _bufs]


def _ptrs(*addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


def _stats(zh=2, zw=2, clip=0.98, dark=1 / 64):
    return _native.Statistics(zh, zw, clip, dark)


GOOD = dict(n=1, H=H, W=W, kind=MI_RAW_16U, ids=0, pattern=0, levels=None, defects=None, src=_addr[0], out=_addr[1],
            stats=_stats(), dtype=MI_F32)

_defect = _native.Defects(_addr[2], 3, None)                # three listed pixels and no mask
_negative = _native.Defects(_addr[2], -1, None)
INF, NAN = float("inf"), float("nan")


def _batch(L, a):
    return L.mi_isp_statistics_raw_batch(_ptrs(a["src"]), _ptrs(a["out"]), a["n"], a["H"], a["W"], a["kind"], a["ids"],
                                         a["pattern"], a["levels"],
                                         None if a["defects"] is None else _ptrs(ctypes.addressof(a["defects"])),
                                         a["stats"], None)


def _single(L, a):
    return L.mi_isp_statistics_raw(a["src"], a["out"], a["H"], a["W"], a["kind"], a["ids"], a["pattern"], a["levels"],
                                   a["defects"], a["stats"], None)


def _cfa(L, a):
    return L.mi_isp_statistics_cfa(a["src"], a["out"], a["H"], a["W"], a["dtype"], a["pattern"], a["defects"], a["stats"], None)


# the checks every entry point makes: (case name, the one bad argument, the text after "<who>: ")
SETTINGS = [
    ("null_settings", dict(stats=None), "null statistics settings"),
    ("zones_zero", dict(stats=_stats(zh=0)), "statistics zones 0x2 outside 1 .. 32"),
    ("zones_33", dict(stats=_stats(zw=33)), "statistics zones 2x33 outside 1 .. 32"),
    ("clip_zero", dict(stats=_stats(clip=0.0)), "statistics clip 0 must be finite and > 0"),
    ("clip_nan", dict(stats=_stats(clip=NAN)), "statistics clip nan must be finite and > 0"),
    ("clip_inf", dict(stats=_stats(clip=INF)), "statistics clip inf must be finite and > 0"),
    ("dark_negative", dict(stats=_stats(clip=0.5, dark=-0.5)), "statistics dark -0.5 must be finite, >= 0 and below clip 0.5"),
    ("dark_at_clip", dict(stats=_stats(clip=0.5, dark=0.5)), "statistics dark 0.5 must be finite, >= 0 and below clip 0.5"),
    ("dark_nan", dict(stats=_stats(clip=0.5, dark=NAN)), "statistics dark nan must be finite, >= 0 and below clip 0.5"),
    ("pattern", dict(pattern=4), "bad statistics pattern 4"),
    ("negative_shape", dict(H=-2), f"bad statistics shape -2x{W}"),
    ("oversized", dict(H=1 << 22), f"statistics frame {1 << 22}x{W} too large"),
    ("odd_rows", dict(H=5), f"statistics: frames must be even size, got 5x{W}"),
    ("odd_columns", dict(W=7), f"statistics: frames must be even size, got {H}x7"),
    ("too_many_pixels", dict(H=8194, W=8192), "statistics: frame 8194x8192 has more than 2^26 pixels"),
    ("tile_rows", dict(H=(1 << 22) - 2, W=2, stats=_stats(zw=1)), f"statistics: frame {(1 << 22) - 2}x2 has more than 65535 tile rows"),
    ("zone_rows", dict(stats=_stats(zh=3)), f"statistics: zones 3x2 exceed the {H // 2}x{W // 2} quads of the frame"),
    ("zone_columns", dict(stats=_stats(zw=5)), f"statistics: zones 2x5 exceed the {H // 2}x{W // 2} quads of the frame"),
    ("defects_negative", dict(defects=_negative), "statistics: negative defect count -1"),
    ("defects_no_mask", dict(defects=_defect), "statistics: frame 0: defects without a mask"),
    ("unaligned_output", dict(out=_addr[1] + 4), "statistics: the output of frame 0 is not aligned to 8 bytes"),
]
RAW = [
    ("kind", dict(kind=5), "bad statistics source kind 5"),
    ("kind_negative", dict(kind=-1), "bad statistics source kind -1"),
    ("ids_packed16", dict(kind=MI_RAW_PACKED16, ids=1), "statistics: the IDS layout is a packed-12 layout"),
    ("levels_f32", dict(kind=MI_RAW_32F, levels=_native.levels_arg([0] * 4, 100)),
     f"statistics: levels apply to u16 codes only (source kind {MI_RAW_32F})"),
    ("levels_white", dict(kind=MI_RAW_PACKED12, levels=_native.levels_arg([0] * 4, 5000)), "white level 5000 outside (0, 4095]"),
    ("levels_black", dict(levels=_native.levels_arg([0, 0, 200, 0], 100)), "black level 200 of site 2 outside [0, white = 100)"),
    ("null_source", dict(src=None), "statistics: frame 0 has a null pointer"),
    ("null_output", dict(out=None), "statistics: frame 0 has a null pointer"),
]
CFA = [
    ("dtype", dict(dtype=MI_U8), "statistics work dtype must be f16 or f32"),
    ("null_cfa", dict(src=None), "statistics: null pointer"),
    ("null_output", dict(out=None), "statistics: null pointer"),
]
ENTRIES = {"statistics_raw": (_single, SETTINGS + RAW), "statistics_raw_batch": (_batch, SETTINGS + RAW),
           "statistics_cfa": (_cfa, SETTINGS + CFA)}
CASES = [(who, name) for who, (_, cases) in ENTRIES.items() for name, _, _ in cases]


@pytest.mark.parametrize("who,case", CASES, ids=[f"{w}-{c}" for w, c in CASES])
def test_entry_rejects_on_the_host(who, case):
    L = _native.lib()
    entry, cases = ENTRIES[who]
    bad, text = next((b, t) for name, b, t in cases if name == case)
    assert entry(L, {**GOOD, **bad}) == 1
    assert L.mi_isp_last_error() == f"{who}: {text}".encode()


def test_the_batch_entry_checks_its_lists_and_its_count():
    L = _native.lib()
    s = _stats()
    assert L.mi_isp_statistics_raw_batch(None, _ptrs(_addr[1]), 1, H, W, MI_RAW_16U, 0, 0, None, None, s, None) == 1
    assert L.mi_isp_last_error() == b"statistics_raw_batch: statistics: null frame list"
    assert L.mi_isp_statistics_raw_batch(_ptrs(_addr[0]), None, 1, H, W, MI_RAW_16U, 0, 0, None, None, s, None) == 1
    assert L.mi_isp_last_error() == b"statistics_raw_batch: statistics: null frame list"
    assert L.mi_isp_statistics_raw_batch(_ptrs(_addr[0]), _ptrs(_addr[1]), -1, H, W, MI_RAW_16U, 0, 0, None, None, s, None) == 1
    assert L.mi_isp_last_error() == b"statistics_raw_batch: statistics with -1 frames"
    two = _ptrs(_addr[1], _addr[1] + 2)
    assert L.mi_isp_statistics_raw_batch(_ptrs(_addr[0], _addr[0]), two, 2, H, W, MI_RAW_16U, 0, 0, None, None, s, None) == 1
    assert L.mi_isp_last_error() == b"statistics_raw_batch: statistics: the output of frame 1 is not aligned to 8 bytes"
    assert L.mi_isp_statistics_raw_batch(_ptrs(_addr[0]), _ptrs(_addr[1]), 1, 6, 6, MI_RAW_PACKED12, 0, 0, None, None,
                                         _stats(zh=4), None) == 1
    assert L.mi_isp_last_error() == b"statistics_raw_batch: statistics: zones 4x2 exceed the 3x3 quads of the frame"


def test_nothing_to_do_is_no_error():
    """n == 0 and H * W == 0 succeed without a launch - and without a look at the pointers or the zone grid."""
    L = _native.lib()
    s = _stats(zh=32, zw=32)
    assert L.mi_isp_statistics_raw_batch(None, None, 0, H, W, MI_RAW_16U, 0, 0, None, None, s, None) == 0
    assert L.mi_isp_statistics_raw_batch(None, None, 3, 0, W, MI_RAW_16U, 0, 0, None, None, s, None) == 0
    assert L.mi_isp_statistics_raw(None, None, H, 0, MI_RAW_PACKED12, 0, 0, None, None, s, None) == 0
    assert L.mi_isp_statistics_cfa(None, None, 0, 0, MI_F16, 0, None, s, None) == 0
    assert L.mi_isp_statistics_cfa(None, None, 0, 0, MI_F16, 0, None, None, None) == 1      # (the settings are checked first)


def test_every_entry_has_every_case():
    assert len(CASES) == 2 * (len(SETTINGS) + len(RAW)) + len(SETTINGS) + len(CFA) == 2 * 29 + 24


def test_the_host_only_queries_reject_with_their_full_texts():
    L = _native.lib()
    s = _stats()
    assert L.mi_isp_statistics_geometry(None) == 1
    assert L.mi_isp_last_error() == b"statistics_geometry: null pointer"
    for bad in (None, _stats(zh=0), _stats(zw=33)):
        assert L.mi_isp_statistics_words(bad) == -1
        assert L.mi_isp_last_error() == b"statistics_words: statistics zones outside 1 .. 32"
    assert L.mi_isp_statistics_direct_blocks(1, 5, W, s) == -1
    assert L.mi_isp_last_error() == f"statistics_direct_blocks: statistics: frames must be even size, got 5x{W}".encode()
    assert L.mi_isp_statistics_direct_blocks(1, H, W, _stats(zh=3)) == -1
    assert L.mi_isp_last_error() == b"statistics_direct_blocks: statistics: zones 3x2 exceed the 2x4 quads of the frame"
    assert L.mi_isp_statistics_direct_blocks(1, H, W, None) == -1
    assert L.mi_isp_last_error() == b"statistics_direct_blocks: null statistics settings"
    assert L.mi_isp_statistics_direct_blocks(33, H, W, s) == -1
    assert L.mi_isp_last_error() == b"statistics_direct_blocks: statistics: a launch takes at most 32 frames, got 33"
    for n, h, w in ((0, H, W), (33, H, W), (1, 0, W), (1, H, -2)):
        assert L.mi_isp_statistics_strip(n, h, w) == -1
        assert L.mi_isp_last_error() == f"statistics_strip: statistics: a launch of {n} frames of {h}x{w}".encode()
