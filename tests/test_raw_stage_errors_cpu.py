"""The raw stages' host checks without a GPU: each of the five `_raw_batch` entry points rejects one bad argument at a time
before any launch, with its return code and its full error text.  The addresses are made up (host buffers): nothing is
launched or dereferenced.  The texts are the entry points' behaviour, stage by stage: denoise has no "<stage>: " prefix,
exposure merge counts brackets."""
import ctypes

import pytest

from taichi_image_amd import _native
from taichi_image_amd._native import MI_F16, MI_RAW_16U, MI_RAW_32F, MI_RAW_PACKED12, MI_RAW_PACKED16

H, W = 4, 8
_bufs = [(ctypes.c_uint8 * 4096)() for _ in range(6)]       # disjoint planes, each larger than any 4 x 8 frame
_addr = [ctypes.addressof(b) for b in _bufs]


def _ptrs(*addresses):
    return (ctypes.c_void_p * len(addresses))(*addresses)


GOOD = dict(n=1, H=H, W=W, kind=MI_RAW_16U, ids=0, work=MI_F16, pattern=0, levels=None, shading=None, defects=None, plain=0,
            src=_addr[0], src2=_addr[1], dst=_addr[2], hist_in=_addr[3], hist_out=_addr[4])


def _denoise(L, a):
    s = _native.Denoise(1.0, 0.01, 1.0, 1.0, 1)
    return L.mi_isp_denoise_raw_batch(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], a["kind"], a["ids"], a["work"],
                                      a["levels"], a["shading"], a["defects"], ctypes.byref(s), None)


def _highlights(L, a):
    s = _native.Highlights(0, 1.0, (ctypes.c_float * 3)(2.0, 1.0, 1.5), None)
    return L.mi_isp_highlights_raw_batch(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], a["kind"], a["ids"],
                                         a["work"], a["pattern"], a["levels"], a["shading"], a["defects"], ctypes.byref(s),
                                         a["plain"], None)


def _chromatic(L, a):
    one = (ctypes.c_double * 3)(1.0, 0.0, 0.0)                # the identity: no shift at any frame size
    s = _native.Chromatic(1.5, 3.5, 4.0, one, one)
    return L.mi_isp_chromatic_raw_batch(_ptrs(a["src"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], a["kind"], a["ids"],
                                        a["work"], a["pattern"], a["levels"], a["shading"], a["defects"], ctypes.byref(s),
                                        a["plain"], None)


def _temporal(L, a):
    s = _native.Temporal(1.0, 0.01, 3.0, 0.5)
    return L.mi_isp_temporal_raw_batch(_ptrs(a["src"]), _ptrs(a["hist_in"]), _ptrs(a["hist_out"]), _ptrs(a["dst"]), a["n"],
                                       a["H"], a["W"], a["kind"], a["ids"], a["work"], a["levels"], a["shading"], a["defects"],
                                       ctypes.byref(s), a["plain"], None)


def _merge(L, a):
    s = _native.ExposureMerge(2, (ctypes.c_float * 4)(1.0, 4.0, 0.0, 0.0), 1.0, 0.01, 0.9, 0.5, 3.0)
    return L.mi_isp_merge_raw_batch(_ptrs(a["src"], a["src2"]), _ptrs(a["dst"]), a["n"], a["H"], a["W"], a["kind"], a["ids"],
                                    a["work"], a["levels"], a["shading"], a["defects"], ctypes.byref(s), a["plain"], None)


# entry, who, the noun of its texts, their "<stage>: " prefix, what it counts, the null pointer of its case and that text
STAGES = {
    "denoise": (_denoise, "denoise_raw_batch", "denoise", "", "frame", "src", "frame 0 has a null pointer"),
    "highlights": (_highlights, "highlights_raw_batch", "highlights", "highlights: ", "frame", "src",
                   "frame 0 has a null pointer"),
    "chromatic": (_chromatic, "chromatic_raw_batch", "chromatic aberration", "chromatic aberration: ", "frame", "src",
                  "frame 0 has a null pointer"),
    "temporal": (_temporal, "temporal_raw_batch", "temporal", "temporal: ", "frame", "src", "frame 0 has a null pointer"),
    "merge": (_merge, "merge_raw_batch", "exposure merge", "exposure merge: ", "bracket", "src2",
              "bracket 0 has a null frame 1"),
}

_grid = _native.Shading(_addr[5], 1, 2, 2)
_defect = _native.Defects(_addr[5], 3, None)                 # three listed pixels and no mask
_defect_list = _ptrs(ctypes.addressof(_defect))


def _cases(noun, prefix, item, null_key, null_text):
    """(case name, the one bad argument, the text after "<who>: ")"""
    return [
        ("kind", dict(kind=5), f"bad {noun} source kind 5"),
        ("odd_packed", dict(kind=MI_RAW_PACKED12, H=3), f"{prefix}packed frames must be even size, got 3x{W}"),
        ("ids_packed16", dict(kind=MI_RAW_PACKED16, ids=1), f"{prefix}the IDS layout is a packed-12 layout"),
        ("levels_f32", dict(kind=MI_RAW_32F, levels=_native.levels_arg([0] * 4, 100)),
         f"{prefix}levels apply to u16 codes only (source kind {MI_RAW_32F})"),
        ("plain_grid", dict(plain=1, shading=_grid), f"{prefix}the plain f32 output takes no shading grid"),
        ("defects_no_mask", dict(defects=_defect_list), f"{prefix}{item} 0: defects without a mask"),
        ("null_frame", {null_key: None}, f"{prefix}{null_text}"),
        ("oversized", dict(H=1 << 22), f"{noun} frame {1 << 22}x{W} too large"),
    ]


CASES = [(stage, name) for stage, v in STAGES.items() for name, _, _ in _cases(*v[2:])
         if not (stage == "denoise" and name == "plain_grid")]         # denoise has no plain output


@pytest.mark.parametrize("stage,case", CASES, ids=[f"{s}-{c}" for s, c in CASES])
def test_raw_batch_entry_rejects_on_the_host(stage, case):
    L = _native.lib()
    entry, who, *texts = STAGES[stage]
    bad, text = next((b, t) for name, b, t in _cases(*texts) if name == case)
    assert entry(L, {**GOOD, **bad}) == 1
    assert L.mi_isp_last_error() == f"{who}: {text}".encode()


def test_every_stage_has_every_case():
    assert len(CASES) == 5 * 8 - 1
