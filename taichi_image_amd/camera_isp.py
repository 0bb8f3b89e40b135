"""Stateful camera ISP -- call surface of taichi_image/camera_isp.py (Camera16 / Camera32).

load (unpack/normalise) -> demosaic(+colour matrix) -> resize; rolling metering statistics;
Reinhard / linear tonemap to u8; orientation transform.  All device work is HIP
(csrc/): the load path is one fused tile kernel over the packed frame, the tonemaps are
two-pass elementwise kernels with wave-shuffle reductions.

Deliberate differences from the reference (see DESIGN.md "quirks"):
 * `_process_image` forwards `self.bayer_pattern` (the reference drops it and always demosaics
   RGGB, camera_isp.py:372); identical for RGGB.  `reference_quirks=True` reproduces the reference.
 * tonemap parameters are runtime floats (the reference re-JITs per value).
 * NaN / out-of-range float->u8 casts are defined (0 / saturate) where the reference is undefined.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional

import numpy as np
import torch

from . import _native, bayer, interpolate, packed, types
from . import defects as _defects
from . import denoise as _dn
from . import highlights as _hl
from . import dynamic_defects as _ddp
from . import green_equalize as _geq
from . import statistics as _st
from . import chromatic as _ca
from . import temporal as _tn
from . import exposure_merge as _em
from . import lens as _lens
from . import sharpen as _shp
from . import chroma_denoise as _cdn
from . import luma_denoise as _ydn
from . import color_lut as _clut
from . import local_contrast as _lc
from . import local_tonemap as _ltm
from . import demosaic as _dm
from . import resample as _rs
from . import white_balance as _wb
from . import distributed as _dist

_LEAVE = object()                            # set(statistics=): "not given" (None turns the option off)

# the optional stages of Camera16 / Camera32: (constructor / set() argument, attribute, checker), in the order set() checks them
_OPTIONAL_STAGES = (
    ("raw_denoise", "_raw_denoise", _dn.check_raw_denoise),
    ("highlights", "_highlights", _hl.check_highlights),
    ("dynamic_defects", "_dynamic_defects", _ddp.check_dynamic_defects),
    ("green_equalize", "_green_equalize", _geq.check_green_equalize),
    ("statistics", "_statistics", _st.check_statistics),
    ("chromatic_aberration", "_chromatic", _ca.check_chromatic_aberration),
    ("temporal_denoise", "_temporal", _tn.check_temporal_denoise),
    ("exposure_merge", "_merge", _em.check_exposure_merge),
    ("local_tonemap", "_ltm", _ltm.check_local_tonemap),
    ("sharpen", "_sharpen", _shp.check_sharpen),
    ("local_contrast", "_local_contrast", _lc.check_local_contrast),
    ("chroma_denoise", "_chroma_denoise", _cdn.check_chroma_denoise),
    ("luma_denoise", "_luma_denoise", _ydn.check_luma_denoise),
    ("color_lut", "_color_lut", _clut.check_color_lut),
    ("demosaic", "_demosaic", _dm.check_demosaic),
    ("resample", "_resample", _rs.check_resample),
)

default_cc = np.array([      # camera_isp.py:230-234
    [1.75, -0.25, -0.30],
    [-0.10, 1.40, -0.30],
    [-0.05, -0.55, 2.10],
])


def _typecheck(name, value, kinds, optional=False):
    if optional and value is None:
        return
    if isinstance(value, bool) and bool not in (kinds if isinstance(kinds, tuple) else (kinds,)):
        raise TypeError(f"{name} must be {kinds}, got bool")
    if not isinstance(value, kinds):
        raise TypeError(f"{name} must be {kinds}, got {type(value).__name__}")


def _check_levels(black_level, white_level, bits=16):
    """The sensor levels as the kernels take them: (black per CFA site (4 ints), white), or None without levels.
    ValueError unless they are integers with 0 <= black_s < white <= 2**bits - 1; white defaults to the full scale."""
    if black_level is None and white_level is None:
        return None
    top = (1 << bits) - 1

    def _int(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what} must be an integer, got {type(v).__name__}")
        return int(v)

    if black_level is None:
        black = [0, 0, 0, 0]
    elif isinstance(black_level, (list, tuple, np.ndarray)):
        if len(black_level) != 4:
            raise ValueError(f"black_level must be one int or 4 (one per CFA site), got {len(black_level)}")
        black = [_int(b, "black_level") for b in black_level]
    else:
        black = [_int(black_level, "black_level")] * 4
    white = top if white_level is None else _int(white_level, "white_level")
    if not 0 < white <= top:
        raise ValueError(f"white_level {white} outside (0, {top}] for a {bits}-bit source")
    for b in black:
        if not 0 <= b < white:
            raise ValueError(f"black_level {b} outside [0, white_level = {white})")
    return black, white


def _check_shading(lens_shading):
    """A lens shading grid as the kernels take it: a contiguous (sites, Gh, Gw) f32 numpy array, sites 1 or 4, from a
    (Gh, Gw) or (4, Gh, Gw) numpy array or torch tensor.  ValueError unless 2 <= Gh, Gw <= 64 and every gain is finite
    and within [0, 16].  DESIGN.md 3, "Lens shading"."""
    if isinstance(lens_shading, torch.Tensor):
        g = lens_shading.detach().to("cpu", torch.float64).numpy()
    elif isinstance(lens_shading, np.ndarray):
        g = np.asarray(lens_shading, dtype=np.float64)
    else:
        raise ValueError(f"lens_shading must be a numpy array or a torch tensor, got {type(lens_shading).__name__}")
    if g.ndim == 2:
        g = g[None]
    if g.ndim != 3 or g.shape[0] not in (1, 4) or (lens_shading.ndim == 3 and g.shape[0] != 4):
        raise ValueError(f"lens_shading must be (Gh, Gw) or (4, Gh, Gw), got shape {tuple(lens_shading.shape)}")
    if not (2 <= g.shape[1] <= 64 and 2 <= g.shape[2] <= 64):
        raise ValueError(f"lens_shading grid {g.shape[1]} x {g.shape[2]} outside 2 .. 64 nodes per axis")
    if not np.all(np.isfinite(g)):
        raise ValueError("lens_shading gains must be finite")
    if g.min() < 0 or g.max() > 16:
        raise ValueError(f"lens_shading gains must be within [0, 16], got [{g.min()}, {g.max()}]")
    return np.ascontiguousarray(g, dtype=np.float32)


def lens_shading_from_flat(codes, grid=(17, 13), black_level=0, per_site=True):
    """A lens shading grid from a flat-field capture (calibration, off the hot path; torch on the codes' device, or numpy).

    codes: (H, W) raw codes (`packed.decode12(..., scaled=False)` gives them).  grid: (Gh, Gw) nodes, node (i, j) at raw
    pixel (i * (H-1)/(Gh-1), j * (W-1)/(Gw-1)).  For each CFA site s = (row & 1) * 2 + (col & 1) and node: the mean of
    max(code - black_s, 0) over the site's pixels within half a cell of the node (clipped to the frame), and
    gain = max(the site's means) / mean.  per_site=False pools the four sites into one (Gh, Gw) grid.  Returns a
    (4, Gh, Gw) grid (or (Gh, Gw)), f32, a torch tensor for torch codes and a numpy array otherwise; ValueError for a node
    whose mean is zero."""
    as_numpy = not isinstance(codes, torch.Tensor)
    c = torch.from_numpy(np.asarray(codes)) if as_numpy else codes
    if c.ndim != 2:
        raise ValueError(f"codes must be (H, W), got shape {tuple(c.shape)}")
    gh, gw = (int(grid[0]), int(grid[1]))
    if not (2 <= gh <= 64 and 2 <= gw <= 64):
        raise ValueError(f"grid {gh} x {gw} outside 2 .. 64 nodes per axis")
    black = list(black_level) if isinstance(black_level, (list, tuple, np.ndarray)) else [black_level] * 4
    if len(black) != 4:
        raise ValueError(f"black_level must be one value or 4 (one per CFA site), got {len(black)}")
    H, W = c.shape
    c = c.to(torch.float64)
    sums = torch.zeros((4, gh, gw), dtype=torch.float64, device=c.device)
    counts = torch.zeros((4, gh, gw), dtype=torch.float64, device=c.device)

    def ranges(n_px, n_nodes, off):
        # per node: the index range [lo, hi) into the site's pixels (off, off + 2, ...) within half a cell of the node
        cell = (n_px - 1) / (n_nodes - 1)
        pos = np.arange(n_nodes) * cell
        lo = np.clip(np.ceil(pos - cell / 2), 0, n_px - 1)
        hi = np.clip(np.floor(pos + cell / 2), 0, n_px - 1)
        klo = np.ceil((lo - off) / 2).astype(np.int64)
        khi = np.floor((hi - off) / 2).astype(np.int64) + 1
        return np.maximum(klo, 0), np.maximum(khi, np.maximum(klo, 0))

    for s in range(4):
        r0, c0 = s >> 1, s & 1
        x = (c[r0::2, c0::2] - float(black[s])).clamp_min(0.0)
        integ = torch.zeros((x.shape[0] + 1, x.shape[1] + 1), dtype=torch.float64, device=c.device)
        integ[1:, 1:] = x.cumsum(0).cumsum(1)
        rlo, rhi = (torch.from_numpy(v).to(c.device) for v in ranges(H, gh, r0))
        clo, chi = (torch.from_numpy(v).to(c.device) for v in ranges(W, gw, c0))
        rhi = rhi.clamp_max(x.shape[0]); chi = chi.clamp_max(x.shape[1])
        R0, C0, R1, C1 = rlo[:, None], clo[None, :], rhi[:, None], chi[None, :]
        sums[s] = integ[R1, C1] - integ[R0, C1] - integ[R1, C0] + integ[R0, C0]
        counts[s] = ((R1 - R0).clamp_min(0) * (C1 - C0).clamp_min(0)).to(torch.float64)
    if not per_site:
        sums, counts = sums.sum(0, keepdim=True), counts.sum(0, keepdim=True)
    if bool((counts == 0).any()):
        raise ValueError("lens_shading_from_flat: a node has no pixel of its site within half a cell (grid too fine)")
    means = sums / counts
    if bool((means == 0).any()):
        raise ValueError("lens_shading_from_flat: a node's flat-field mean is zero")
    gains = (means.amax(dim=(1, 2), keepdim=True) / means).to(torch.float32)
    if not per_site:
        gains = gains[0]
    return gains.cpu().numpy() if as_numpy else gains


class MeteringTimeout(RuntimeError):
    """The grid barrier of an earlier one-launch update_metering on this device timed out (something else held compute
    units of the GPU for about a second).  That call left the metrics as they were - bounds folded from half of the blocks
    must never enter the rolling average - so everything tone-mapped with them since is suspect.  Raised by the NEXT
    update_metering / tonemap call (one host read of the device's mailbox, no synchronisation)."""


class TonemapTimeout(RuntimeError):
    """The grid-wide wait of an earlier one-launch process_packed12 on this device (max_out, camera_isp.py:213) timed out:
    the u8 outputs of that call are invalid.  Raised by the next metering / tonemap call (a host read of the mailbox)."""


def _raise_resident_faults(L, device):
    """MeteringTimeout / TonemapTimeout for a timeout an earlier resident-grid launch on `device` left in its mailbox word
    (a host read each, no synchronisation; the words are cleared)."""
    with torch.cuda.device(device):
        if L.mi_isp_metering_faults(1):
            raise MeteringTimeout("an earlier update_metering on this device timed out at its grid barrier: its "
                                  "metrics were left unchanged and outputs tone-mapped with them are invalid")
        if L.mi_isp_camera_group_faults(1):
            raise TonemapTimeout("an earlier process_packed12 on this device timed out waiting for an image's "
                                 "max_out: the outputs of that call are invalid")


def _version_of(t):
    """torch's write counter of a tensor, None where there is none (inference tensors do not track one)."""
    try:
        return t._version
    except RuntimeError:
        return None


def _tag_subsample(rgb, sub, stride):
    """Hang the dense metering subsample the load kernel left (`rgb[::stride, ::stride]`) on the image.  The tag is valid
    while the image's version counter stands still: torch writes move it, the library's own in-place writes move it
    explicitly (_written_in_place).  A tensor without a counter (created under torch.inference_mode(), as the reference's
    bench does, bench/camera_isp.py:53) gets no tag - update_metering then gathers from the image itself."""
    v = _version_of(rgb)
    if v is not None:
        rgb._mi_metering_sub = (sub, stride, v)


def _valid_subsample(im, stride):
    tag = getattr(im, "_mi_metering_sub", None)
    if tag is None or tag[1] != stride or tag[2] != _version_of(im):
        return None
    return tag[0]


def _written_in_place(images):
    """The library has overwritten these images through their raw pointers (Reinhard pass 1 writes the mapped values p
    back, camera_isp.py:211): what torch cannot see is made visible - the version counter moves (views and autograd see
    a write) and a metering subsample taken before the write is dropped, so the next update_metering meters the
    MUTATED image as the reference does (camera_isp.py:168-175 on the image of :211)."""
    for im in images:
        if getattr(im, "_mi_metering_sub", None) is not None:
            del im._mi_metering_sub
        if _version_of(im) is not None:
            torch.autograd.graph.increment_version(im)


def camera_isp(name: str, dtype=types.f32):
    """camera_isp.py:75-418: class factory specialised on the working dtype."""
    dtype = types.as_dtype(dtype)
    torch_dtype = types.ti_to_torch[dtype]

    def _check_image(image, what="image"):
        if not isinstance(image, torch.Tensor):
            raise TypeError(f"{what} must be a torch.Tensor")
        assert image.ndim == 3 and image.shape[2] == 3, f"{what} must be (H, W, 3)"
        assert image.dtype == torch_dtype, f"{what} must be {torch_dtype}, got {image.dtype}"
        assert image.is_cuda and image.is_contiguous(), f"{what} must be a contiguous device tensor"

    def reinhard_kernel(image, output, metering, gamma, intensity, light_adapt, color_adapt,
                        transform=interpolate.ImageTransform.none):
        """camera_isp.py:177-218.  Mutates `image` (p written back in place), fills `output`."""
        _check_image(image)
        H, W = image.shape[:2]
        ws = _native.workspace(H, W, image.device)
        _native.check(_native.lib().mi_isp_reinhard(
            image.data_ptr(), output.data_ptr(), H, W, dtype.code, metering.data_ptr(), float(gamma),
            float(intensity), float(light_adapt), float(color_adapt), interpolate.transform_code(transform),
            ws.data_ptr(), _native.stream_ptr(image.device)))
        _written_in_place([image])

    def linear_kernel(image, output, metering, gamma, transform=interpolate.ImageTransform.none):
        """camera_isp.py:220-227."""
        _check_image(image)
        H, W = image.shape[:2]
        ws = _native.workspace(H, W, image.device)
        _native.check(_native.lib().mi_isp_linear(
            image.data_ptr(), output.data_ptr(), H, W, dtype.code, metering.data_ptr(), float(gamma),
            interpolate.transform_code(transform), ws.data_ptr(), _native.stream_ptr(image.device)))

    def _check_transform(images, transform):
        """interpolate.transform's rule, checked before a tonemap touches the metering state: the C entries reject a
        non-square transverse too, but only after update_metering has already moved the state."""
        if transform == interpolate.ImageTransform.transverse:
            for im in images:
                if isinstance(im, torch.Tensor) and im.ndim >= 2:
                    assert im.shape[0] == im.shape[1], "transverse is only defined for square images"

    def _out_shape(image, transform):
        H, W = image.shape[:2]
        if transform in (interpolate.ImageTransform.rotate_90, interpolate.ImageTransform.rotate_270,
                         interpolate.ImageTransform.transpose):
            return (W, H, 3)
        return (H, W, 3)

    class ISP():
        def __init__(self, bayer_pattern: bayer.BayerPattern,
                     scale: Optional[float] = None,
                     resize_width: int = 0,
                     moving_alpha=0.1,
                     correct_colors: bool = False,
                     white_balance: np.ndarray = np.array([1.8, 1.0, 2.1]),
                     color_correction: np.ndarray = default_cc,
                     transform: interpolate.ImageTransform = interpolate.ImageTransform.none,
                     device: torch.device = torch.device('cuda', 0),
                     metering_stride: int = 8,
                     process_group=None,
                     reference_quirks: bool = False,
                     black_level=None,
                     white_level: Optional[int] = None,
                     lens_shading=None,
                     auto_white_balance=False,
                     raw_denoise=None,
                     sharpen=None,
                     local_contrast=None,
                     chroma_denoise=None,
                     color_lut=None,
                     highlights=None,
                     chromatic_aberration=None,
                     temporal_denoise=None,
                     exposure_merge=None,
                     local_tonemap=None,
                     luma_denoise=None,
                     demosaic=None,
                     resample=None,
                     dynamic_defects=None,
                     green_equalize=None,
                     statistics=None):
            _typecheck("bayer_pattern", bayer_pattern, bayer.BayerPattern)
            _typecheck("scale", scale, float, optional=True)
            _typecheck("resize_width", resize_width, int)
            _typecheck("correct_colors", correct_colors, bool)
            _typecheck("white_balance", white_balance, np.ndarray)
            _typecheck("color_correction", color_correction, np.ndarray)
            _typecheck("transform", transform, interpolate.ImageTransform)
            _typecheck("device", device, torch.device)
            _typecheck("metering_stride", metering_stride, int)
            assert scale is None or resize_width == 0, "Cannot specify both scale and resize_width"
            _check_levels(black_level, white_level)
            shading = None if lens_shading is None else _check_shading(lens_shading)
            awb = _wb.check_auto_white_balance(auto_white_balance)
            if awb is not None:
                _wb.check_seed(white_balance)
            raw_denoise = _dn.check_raw_denoise(raw_denoise)
            highlights = _hl.check_highlights(highlights)
            dynamic_defects = _ddp.check_dynamic_defects(dynamic_defects)
            green_equalize = _geq.check_green_equalize(green_equalize)
            statistics = _st.check_statistics(statistics)
            chromatic_aberration = _ca.check_chromatic_aberration(chromatic_aberration)
            temporal_denoise = _tn.check_temporal_denoise(temporal_denoise)
            exposure_merge = _em.check_exposure_merge(exposure_merge)
            local_tonemap = _ltm.check_local_tonemap(local_tonemap)
            sharpen = _shp.check_sharpen(sharpen)
            local_contrast = _lc.check_local_contrast(local_contrast)
            chroma_denoise = _cdn.check_chroma_denoise(chroma_denoise)
            luma_denoise = _ydn.check_luma_denoise(luma_denoise)
            color_lut = _clut.check_color_lut(color_lut)
            demosaic = _dm.check_demosaic(demosaic)
            resample = _rs.check_resample(resample)

            self.bayer_pattern = bayer_pattern
            # reference_quirks=True: demosaic as the reference does - ISP._process_image calls bayer_to_rgb WITHOUT its
            # pattern (camera_isp.py:371-373), so every camera is demosaiced as RGGB whatever bayer_pattern says.  For
            # comparisons against the reference's own outputs; the default honours the pattern.
            _typecheck("reference_quirks", reference_quirks, bool)
            self.reference_quirks = reference_quirks
            self.moving_alpha = moving_alpha
            self.scale = scale
            self.resize_width = resize_width
            self.transform = transform
            self.metering_stride = metering_stride

            self.correct_colors = correct_colors
            self.white_balance = white_balance
            self.color_correction = color_correction

            # sensor levels (an extension): black per CFA site of the raw frame ((row & 1) * 2 + (col & 1), whatever the
            # pattern), white; both None: no levels, the loaders run exactly as without them.  DESIGN.md 3.
            self.black_level = black_level
            self.white_level = white_level

            self.metrics = None
            self.device = device
            # lens shading (an extension): a private (sites, Gh, Gw) f32 grid on the device, uploaded once; None: no
            # shading, the loaders run exactly as without it.  Grids a later set() replaced by another shape, or removed,
            # stay referenced in _shading_retired for the ISP's lifetime, so no queued or captured launch reads a freed
            # grid (a grid is at most 64 KB).  DESIGN.md 3, INTEGRATION.md.
            self._shading = None if shading is None else torch.from_numpy(shading).to(device)
            self._shading_retired = []
            # one-process-per-GPU sharding: statistics are all-reduced over this group (RCCL)
            self.process_group = process_group
            # auto white balance (an extension): the AutoWhiteBalance in effect, or None.  On, it owns four device tensors:
            # the pending statistics (5 i64: the sums of the four CFA sites and the quad count), the gray-world state (4
            # f64: S_R, S_G, S_B, valid), the gains (3 f32) and the effective grid E (4 x Gh x Gw f32) that the loaders
            # apply in place of the user's grid.  Replaced or dropped tensors stay referenced in _awb_retired for the
            # ISP's lifetime, as _shading_retired.  DESIGN.md 3, "Auto white balance".
            self._awb = None
            self._awb_E = None
            self._awb_retired = []
            if awb is not None:
                self._awb_seed(awb)
            # raw noise reduction (an extension): the RawDenoise of this sensor, or None (the loaders run exactly as
            # without it).  DESIGN.md 3, "Raw noise reduction".
            self._raw_denoise = raw_denoise
            # highlight reconstruction (an extension): the Highlights the loaders apply to clipped raw pixels, or None (the
            # loaders run exactly as without it).  DESIGN.md 3, "Highlight reconstruction".
            self._highlights = highlights
            # dynamic defects (an extension): the DynamicDefects the loaders detect and replace defective raw pixels with,
            # without a map, or None (the loaders run exactly as without it).  DESIGN.md 3, "Dynamic defects".
            self._dynamic_defects = dynamic_defects
            # green equalisation (an extension): the GreenEqualize the loaders balance the two green phases with, or None
            # (the loaders run exactly as without it).  DESIGN.md 3, "Green equalisation".
            self._green_equalize = green_equalize
            # frame statistics (an extension): the Statistics the loaders measure every raw frame with, or None (the
            # loaders run exactly as without it); frame_statistics: the result of the last loader call, one FrameStatistics
            # per frame (after a bracket loader one list per bracket with one entry per exposure), None with the option
            # off.  A side output: no image, no route and no raw stage depends on it.  DESIGN.md 3, "Frame statistics".
            self._statistics = statistics
            self.frame_statistics = None
            # chromatic aberration (an extension): the ChromaticAberration the loaders correct on the CFA, or None (the
            # loaders run exactly as without it).  DESIGN.md 3, "Chromatic aberration".
            self._chromatic = chromatic_aberration
            # temporal noise reduction (an extension): the TemporalDenoise the loaders apply against the caller's
            # TemporalHistory objects (history=), or None (the loaders run exactly as without it).  The ISP holds no
            # per-camera state of its own.  DESIGN.md 3, "Temporal noise reduction".
            self._temporal = temporal_denoise
            # exposure merge (an extension): the ExposureMerge the bracket loaders apply to the E frames of each bracket,
            # or None (the loaders run exactly as without it).  The stage has no state.  DESIGN.md 3, "Exposure merge".
            self._merge = exposure_merge
            # local tone mapping (an extension): the LocalTonemap every loader applies in place to the image it returns,
            # behind demosaic, resize, lens remap and defect fix-up, or None (the loaders run exactly as without it).
            # DESIGN.md 3, "Local tone mapping".
            self._ltm = local_tonemap
            # output sharpening (an extension): the Sharpen applied to every u8 output of the tonemaps, or None (the
            # tonemaps run exactly as without it).  DESIGN.md 3, "Output sharpening".
            self._sharpen = sharpen
            # local contrast (an extension): the LocalContrast applied in place to every u8 output of the tonemaps, before
            # sharpening, or None (the tonemaps run exactly as without it).  DESIGN.md 3, "Local contrast".
            self._local_contrast = local_contrast
            # chroma noise reduction (an extension): the ChromaDenoise applied to every u8 output of the tonemaps, before
            # local contrast and sharpening, or None (the tonemaps run exactly as without it).  DESIGN.md 3, "Chroma noise
            # reduction".
            self._chroma_denoise = chroma_denoise
            # luma noise reduction (an extension): the LumaDenoise applied to every u8 output of the tonemaps, behind chroma
            # noise reduction and before local contrast and sharpening, or None (the tonemaps run exactly as without it).
            # DESIGN.md 3, "Luma noise reduction".
            self._luma_denoise = luma_denoise
            # 3D colour LUT (an extension): the ColorLut every u8 RGB output of the tonemaps is mapped through, in place,
            # before the other output operators, or None (the tonemaps run exactly as without it).  DESIGN.md 3, "Colour
            # LUT".
            self._color_lut = color_lut
            if color_lut is not None:
                color_lut._device_table(self.device)         # (uploaded now: a captured step finds it on the device)
            # the demosaic (an extension): the Demosaic every loader demosaics with, or None (the 13-tap filter: the loaders
            # run exactly as without it).  DESIGN.md 3, "Directional demosaic".
            self._demosaic = demosaic
            # the resize (an extension): the Resample every loader resizes with, or None (the bilinear resize: the loaders
            # run exactly as without it).  DESIGN.md 3, "Antialiased resize".
            self._resample = resample

        @property
        def _demosaic_pattern(self):
            return bayer.BayerPattern.RGGB if self.reference_quirks else self.bayer_pattern

        def set(self, moving_alpha: Optional[float] = None, resize_width: Optional[int] = None,
                scale: Optional[float] = None,
                correct_colors: Optional[bool] = None,
                white_balance: Optional[np.ndarray] = None,
                color_correction: Optional[np.ndarray] = None,
                transform: Optional[interpolate.ImageTransform] = None,
                black_level=None, white_level: Optional[int] = None, lens_shading=None, auto_white_balance=None,
                raw_denoise=None, sharpen=None, local_contrast=None, chroma_denoise=None, color_lut=None,
                highlights=None, chromatic_aberration=None, temporal_denoise=None, exposure_merge=None,
                local_tonemap=None, luma_denoise=None, demosaic=None, resample=None, dynamic_defects=None,
                green_equalize=None, statistics=_LEAVE):
            """camera_isp.py:270-300; black_level / white_level / lens_shading (the extensions): None leaves the current
            value.  lens_shading=False removes the grid.  A grid of the current shape is copied in place on the device's
            current stream (launches queued before on that stream read the old gains, later ones the new; a captured
            graph reads the new ones at its next replay); a grid of another shape gets a new device tensor and the old
            one stays allocated while the ISP lives.
            auto_white_balance (the extension): None leaves it; False turns it off (the ISP then computes exactly what
            one that never had it does); True or an AutoWhiteBalance turns it on and seeds it: gains f32(white_balance),
            no state, no pending statistics.  white_balance= while it is on seeds it again; lens_shading= while it is on
            rebuilds the effective grid from the new grid and the current gains on the device.
            raw_denoise (the extension): None leaves it, False turns it off, a RawDenoise replaces it.
            sharpen (the extension): None leaves it, False turns it off, a Sharpen replaces it.
            local_contrast (the extension): None leaves it, False turns it off, a LocalContrast replaces it.
            chroma_denoise (the extension): None leaves it, False turns it off, a ChromaDenoise replaces it.
            color_lut (the extension): None leaves it, False turns it off, a ColorLut replaces it.
            highlights (the extension): None leaves it, False turns it off, a Highlights replaces it.
            chromatic_aberration (the extension): None leaves it, False turns it off, a ChromaticAberration replaces it.
            temporal_denoise (the extension): None leaves it, False turns it off, a TemporalDenoise replaces it (the
            histories are the caller's: reset() them when the new settings should not meet old frames).
            exposure_merge (the extension): None leaves it, False turns it off, an ExposureMerge replaces it.
            local_tonemap (the extension): None leaves it, False turns it off, a LocalTonemap replaces it.
            luma_denoise (the extension): None leaves it, False turns it off, a LumaDenoise replaces it.
            demosaic (the extension): None leaves it, False turns it off, a Demosaic replaces it.
            resample (the extension): None leaves it, False turns it off, a Resample replaces it.
            dynamic_defects (the extension): None leaves it, False turns it off, a DynamicDefects replaces it.
            green_equalize (the extension): None leaves it, False turns it off, a GreenEqualize replaces it.
            statistics (the extension): left as it is when not given; None or False turns it off (frame_statistics is None
            again), a Statistics replaces it."""
            if black_level is not None or white_level is not None:
                _check_levels(self.black_level if black_level is None else black_level,
                              self.white_level if white_level is None else white_level)
            shading = None if lens_shading is None or lens_shading is False else _check_shading(lens_shading)
            awb = self._awb if auto_white_balance is None else _wb.check_auto_white_balance(auto_white_balance)
            if awb is not None and (auto_white_balance is not None or white_balance is not None):
                _wb.check_seed(self.white_balance if white_balance is None else white_balance)
            # the optional stages: None leaves one, False turns it off, a value replaces it - every value checked here, before
            # anything is assigned
            given = dict(raw_denoise=raw_denoise, highlights=highlights, chromatic_aberration=chromatic_aberration,
                         temporal_denoise=temporal_denoise, exposure_merge=exposure_merge, local_tonemap=local_tonemap,
                         sharpen=sharpen, local_contrast=local_contrast, chroma_denoise=chroma_denoise,
                         luma_denoise=luma_denoise, color_lut=color_lut, demosaic=demosaic, resample=resample,
                         dynamic_defects=dynamic_defects, green_equalize=green_equalize,
                         statistics=None if statistics is _LEAVE else (False if statistics is None else statistics))
            replaced = {name: check(given[name]) for name, _, check in _OPTIONAL_STAGES
                        if given[name] is not None and given[name] is not False}
            _typecheck("moving_alpha", moving_alpha, float, optional=True)
            _typecheck("resize_width", resize_width, int, optional=True)
            _typecheck("scale", scale, float, optional=True)
            _typecheck("correct_colors", correct_colors, bool, optional=True)
            _typecheck("white_balance", white_balance, np.ndarray, optional=True)
            _typecheck("color_correction", color_correction, np.ndarray, optional=True)
            _typecheck("transform", transform, interpolate.ImageTransform, optional=True)
            if moving_alpha is not None:
                self.moving_alpha = moving_alpha
            if resize_width is not None:
                self.resize_width = resize_width
                self.scale = None
            if scale is not None:
                self.scale = scale
                self.resize_width = 0
            if transform is not None:
                self.transform = transform
            if correct_colors is not None:
                self.correct_colors = correct_colors
            if white_balance is not None:
                self.white_balance = white_balance
            if color_correction is not None:
                self.color_correction = color_correction
            if black_level is not None:
                self.black_level = black_level
            if white_level is not None:
                self.white_level = white_level
            if lens_shading is False:
                if self._shading is not None:
                    self._shading_retired.append(self._shading)
                self._shading = None
            elif shading is not None:
                new = torch.from_numpy(shading)
                if self._shading is not None and tuple(self._shading.shape) == tuple(new.shape):
                    with torch.cuda.device(self.device):
                        self._shading.copy_(new)
                else:
                    if self._shading is not None:
                        self._shading_retired.append(self._shading)
                    self._shading = new.to(self.device)
            for name, attr, _ in _OPTIONAL_STAGES:
                if given[name] is False:
                    setattr(self, attr, None)
                elif replaced.get(name) is not None:
                    setattr(self, attr, replaced[name])
            if self._statistics is None:
                self.frame_statistics = None
            if replaced.get("color_lut") is not None:
                replaced["color_lut"]._device_table(self.device)  # (uploaded now: a captured step finds it on the device)
            if auto_white_balance is not None:
                if awb is None:
                    self._awb_off()
                else:
                    self._awb_seed(awb)
            elif self._awb is not None and white_balance is not None:
                self._awb_seed(self._awb)
            elif self._awb is not None and lens_shading is not None:
                self._awb_rebuild()

        def _awb_seed(self, awb):
            """AWB on with settings awb: the gains f32(white_balance), the state and the pending sums cleared (in place
            when it was on already), E rebuilt."""
            seed = torch.from_numpy(_wb.check_seed(self.white_balance))
            if self._awb is None:
                self._awb_pending = torch.zeros(5, dtype=torch.int64, device=self.device)
                self._awb_state = torch.zeros(4, dtype=torch.float64, device=self.device)
                self._awb_gains = seed.to(self.device)
            else:
                with torch.cuda.device(self.device):
                    self._awb_pending.zero_()
                    self._awb_state.zero_()
                    self._awb_gains.copy_(seed)
            self._awb = awb
            self._awb_rebuild()

        def _awb_off(self):
            if self._awb is not None:
                self._awb_retired += [self._awb_pending, self._awb_state, self._awb_gains, self._awb_E]
            self._awb = None
            self._awb_E = None

        def _awb_rebuild(self):
            """E from the user's grid and the current gains, on the device (a new tensor when its shape changes)."""
            shape = (4,) + (tuple(self._shading.shape[1:]) if self._shading is not None else (2, 2))
            if self._awb_E is None or tuple(self._awb_E.shape) != shape:
                if self._awb_E is not None:
                    self._awb_retired.append(self._awb_E)
                self._awb_E = torch.empty(shape, dtype=torch.float32, device=self.device)
            _native.check(_native.lib().mi_isp_awb_rebuild(
                self._demosaic_pattern.value, self._awb_gains.data_ptr(), _native.shading_arg(self._shading),
                self._awb_E.data_ptr(), _native.stream_ptr(self.device)))

        def _applied_shading(self):
            """The grid the loaders apply: E with AWB on, else the user's grid (or None)."""
            return self._awb_E if self._awb is not None else self._shading

        @property
        def auto_white_balance(self):
            """The AutoWhiteBalance in effect, or None."""
            return self._awb

        @property
        def white_balance_gains(self) -> Optional[torch.Tensor]:
            """The AWB gains (g_R, g_G, g_B), a (3,) f32 device tensor the loaders apply from the next load on (do not
            write it), or None with AWB off."""
            return self._awb_gains if self._awb is not None else None

        def update_white_balance(self):
            """One AWB update from the statistics of every load since the last one (all-gathered over process_group):
            the gray-world state, the gains and E move on the device, the pending sums are cleared.  update_metering (so
            every tonemap and process_packed12) runs it; a no-op with AWB off.  No host synchronisation without a group."""
            if self._awb is None:
                return
            gathered = _dist.all_gather_rows(self._awb_pending, self.process_group)
            _native.check(_native.lib().mi_isp_awb_update(
                gathered.data_ptr(), gathered.shape[0], self._awb_pending.data_ptr(), self._demosaic_pattern.value,
                float(1.0 - self.moving_alpha), self._awb_state.data_ptr(), self._awb_gains.data_ptr(),
                _native.shading_arg(self._shading), self._awb_E.data_ptr(), _native.stream_ptr(self.device)))

        def _awb_stats_cfa(self, src, h, w, mode, lv):
            """With auto white balance on, the statistics of the h x w CFA src (mi_isp_load_convert mode `mode`, levels lv)
            added to the pending sums, on the loads' stream; nothing with it off."""
            if self._awb is not None:
                _native.check(_native.lib().mi_isp_awb_stats_cfa(
                    src.data_ptr(), h, w, mode, lv, _native.shading_arg(self._shading), float(self._awb.clip),
                    float(self._awb.floor), int(self._awb.stride), self._awb_pending.data_ptr(),
                    _native.stream_ptr(self.device)))

        def _awb_stats_packed(self, srcs, h, w, bits, ids_format, lv):
            """The same for the packed frames srcs of one shape, in one launch."""
            if self._awb is not None:
                _native.check(_native.lib().mi_isp_awb_stats_packed(
                    _native.ptr_array(srcs), len(srcs), h, w, bits, int(bool(ids_format)), lv,
                    _native.shading_arg(self._shading), float(self._awb.clip), float(self._awb.floor),
                    int(self._awb.stride), self._awb_pending.data_ptr(), _native.stream_ptr(self.device)))

        def _check_statistics_fits(self, shape):
            """With statistics on, ValueError for a frame shape the statistics cannot take (before anything is uploaded or
            launched)."""
            if self._statistics is not None:
                self._statistics.check_shape(shape)

        def _frame_stats(self, srcs, h, w, kind, ids_format, lv, maps, exposures=None):
            """With statistics on, the statistics of the raw frames srcs (one shape, source kind `kind`, the call's levels
            lv, one DefectMap or None per frame) in one launch per 32 frames behind the loads, on their stream, into
            frame_statistics; nothing with it off.  exposures: the E of a bracket loader, whose srcs hold the E frames
            of each bracket one after another (maps: one per bracket).  Nothing is read to the host."""
            if self._statistics is None:
                self.frame_statistics = None
                return
            e = 1 if exposures is None else exposures
            args = [None if m is None else m._arg(self.device) for m in maps for _ in range(e)]
            out = _st.measure_raw(srcs, h, w, kind, ids_format, self._demosaic_pattern, lv, args, self._statistics,
                                  self.device)
            self.frame_statistics = out if exposures is None else [out[i:i + e] for i in range(0, len(out), e)]

        @property
        def statistics(self) -> Optional[_st.Statistics]:
            """The Statistics the loaders measure with, or None."""
            return self._statistics

        def _raw_stage_on(self):
            """True when a loader of single frames goes through _raw_chain."""
            return (self._highlights is not None or self._chromatic is not None or self._temporal is not None
                    or self._raw_denoise is not None or self._dynamic_defects is not None
                    or self._green_equalize is not None)

        @property
        def raw_denoise(self) -> Optional[_dn.RawDenoise]:
            """The RawDenoise the loaders apply, or None."""
            return self._raw_denoise

        @property
        def highlights(self) -> Optional[_hl.Highlights]:
            """The Highlights the loaders apply, or None."""
            return self._highlights

        @property
        def dynamic_defects(self) -> Optional[_ddp.DynamicDefects]:
            """The DynamicDefects the loaders apply, or None."""
            return self._dynamic_defects

        @property
        def green_equalize(self) -> Optional[_geq.GreenEqualize]:
            """The GreenEqualize the loaders apply, or None."""
            return self._green_equalize

        def _highlights_arg(self):
            """The mi_isp_highlights of a load: the balance gains are the AWB gains on the device with AWB on, else
            f32(white_balance) when the colour matrix carries it (correct_colors), else (1, 1, 1)."""
            if self._awb is not None:
                return self._highlights._arg(gains_dev=self._awb_gains)
            if self.correct_colors:
                return self._highlights._arg(_hl.check_white_balance(self.white_balance))
            return self._highlights._arg()

        @property
        def chromatic_aberration(self) -> Optional[_ca.ChromaticAberration]:
            """The ChromaticAberration the loaders correct, or None."""
            return self._chromatic

        @property
        def temporal_denoise(self) -> Optional[_tn.TemporalDenoise]:
            """The TemporalDenoise the loaders apply against their history= objects, or None."""
            return self._temporal

        @property
        def exposure_merge(self) -> Optional[_em.ExposureMerge]:
            """The ExposureMerge the bracket loaders apply, or None."""
            return self._merge

        def _merge_state(self, bracket, what):
            """ValueError for a single-frame loader while exposure merge is on, or a bracket loader while it is off
            (before anything is uploaded or launched)."""
            if bracket and self._merge is None:
                raise ValueError(f"{what} takes exposure brackets, but exposure_merge is off: pass "
                                 f"exposure_merge=ExposureMerge(...) to the camera or to set()")
            if not bracket and self._merge is not None:
                raise ValueError(f"exposure_merge is on: {what} takes single frames; use the bracket loaders "
                                 f"(load_packed12_bracket, load_packed16_bracket, load_16u_bracket, load_16f_bracket, "
                                 f"load_32f_bracket, load_packed12_bracket_batch, load_packed16_bracket_batch)")

        def _map_args(self, maps):
            """(the mi_isp_defects of each DefectMap of maps, None for None; the array of their addresses for a _batch
            entry point).  The first is what keeps the second's targets alive: hold it through the call."""
            args = [None if m is None else m._arg(self.device) for m in maps]
            return args, (ctypes.c_void_p * len(maps))(*[None if a is None else ctypes.addressof(a) for a in args])

        def _raw_chain(self, srcs, h, w, kind, ids_format, lv, maps, hists=None, brackets=None):
            """The raw chain, the one route of every loader with a raw stage on: the raw stages that are on, in the order
            exposure merge, dynamic defects, highlight reconstruction, chromatic aberration, temporal noise reduction, raw
            noise reduction, green equalisation, one launch each for the raw frames srcs (one shape, source kind `kind`;
            with exposure merge on brackets holds the E frames of each, and srcs their first), then the defect fix-up of
            each frame with a map (maps: one DefectMap or None per frame).  A stage that is not the last writes the plain f32 y, which the next takes as an
            f32 source without levels; the last applies the grid and the cast; all read the same masks.  The temporal
            stage reads and writes the planes of hists (one checked TemporalHistory per frame), which swap once its launch
            was issued; when it is not the last, its new history planes are the y the next stage reads.  Raw noise
            reduction has no plain output of its own: in front of green equalisation it writes an f32 CFA without a grid,
            which is its y.  DESIGN.md 3, "Raw noise reduction", "Highlight reconstruction", "Exposure merge", "Chromatic
            aberration", "Temporal noise reduction", "Dynamic defects" and "Green equalisation"."""
            L = _native.lib()
            stream = _native.stream_ptr(self.device)
            n = len(srcs)
            args, p_maps = self._map_args(maps)
            sh = _native.shading_arg(self._applied_shading())
            pattern = self._demosaic_pattern.value
            ids = int(bool(ids_format))
            stages = []
            if brackets is not None:                     # exposure merge: n * E frames in, n out
                em_arg = self._merge._arg()
                flat = _native.ptr_array([f for b in brackets for f in b])
                stages.append(lambda i, o, k, f, l, s, plain: L.mi_isp_merge_raw_batch(
                    flat, o, n, h, w, k, f, dtype.code, l, s, p_maps, em_arg, plain, stream))
            if self._dynamic_defects is not None:        # (no flag plane: the loaders want the pixels only)
                dd_arg = self._dynamic_defects._arg()
                stages.append(lambda i, o, k, f, l, s, plain: L.mi_isp_dynamic_defects_raw_batch(
                    i, o, n, h, w, k, f, dtype.code, l, s, p_maps, dd_arg, plain, stream, None))
            if self._highlights is not None:
                hl_arg = self._highlights_arg()
                stages.append(lambda i, o, k, f, l, s, plain: L.mi_isp_highlights_raw_batch(
                    i, o, n, h, w, k, f, dtype.code, pattern, l, s, p_maps, hl_arg, plain, stream))
            if self._chromatic is not None:
                ca_arg = self._chromatic._arg((h, w))
                stages.append(lambda i, o, k, f, l, s, plain: L.mi_isp_chromatic_raw_batch(
                    i, o, n, h, w, k, f, dtype.code, pattern, l, s, p_maps, ca_arg, plain, stream))
            if self._temporal is not None:
                stages.append(None)                      # (the stage with histories: below)
            if self._raw_denoise is not None:
                dn_arg = self._raw_denoise._arg()
                stages.append(lambda i, o, k, f, l, s, plain: L.mi_isp_denoise_raw_batch(
                    i, o, n, h, w, k, f, types.f32.code if plain else dtype.code, l, s, p_maps, dn_arg, stream))
            if self._green_equalize is not None:         # (the last stage: directly in front of the demosaic)
                ge_arg = self._green_equalize._arg()
                stages.append(lambda i, o, k, f, l, s, plain: L.mi_isp_green_equalize_raw_batch(
                    i, o, n, h, w, k, f, dtype.code, pattern, l, s, p_maps, ge_arg, plain, stream))
            cfas = [torch.empty((h, w), dtype=torch_dtype, device=self.device) for _ in srcs]
            cur, cur_kind, cur_ids, cur_lv = srcs, kind, ids, lv
            for k, stage in enumerate(stages):
                last = k == len(stages) - 1
                if stage is None:
                    planes = [hist._begin((h, w), self.device) for hist in hists]
                    outs = cfas if last else [new for _, new in planes]
                    _native.check(L.mi_isp_temporal_raw_batch(
                        _native.ptr_array(cur), (ctypes.c_void_p * n)(*[None if old is None else old.data_ptr()
                                                                        for old, _ in planes]),
                        _native.ptr_array([new for _, new in planes]), _native.ptr_array(cfas) if last else None, n, h, w,
                        cur_kind, cur_ids, dtype.code, cur_lv, sh if last else None, p_maps, self._temporal._arg(),
                        int(not last), stream))
                    for hist in hists:
                        hist._commit()
                else:
                    outs = cfas if last else [torch.empty((h, w), dtype=torch.float32, device=self.device) for _ in srcs]
                    _native.check(stage(_native.ptr_array(cur), _native.ptr_array(outs), cur_kind, cur_ids, cur_lv,
                                        sh if last else None, int(not last)))
                cur, cur_kind, cur_ids, cur_lv = outs, _native.MI_RAW_32F, 0, None
            for cfa, a in zip(cfas, args):
                if a is not None:
                    _native.check(L.mi_isp_defects_fix_cfa(cfa.data_ptr(), h, w, dtype.code, a, stream))
            return cfas

        @property
        def demosaic(self) -> Optional[_dm.Demosaic]:
            """The Demosaic the loaders demosaic with, or None (the 13-tap filter)."""
            return self._demosaic

        def _directional(self):
            """True when the loaders take the directional demosaic (Demosaic("malvar") is as without the option)."""
            return self._demosaic is not None and self._demosaic.is_directional

        @property
        def resample(self) -> Optional[_rs.Resample]:
            """The Resample the loaders resize with, or None (the bilinear resize)."""
            return self._resample

        def _antialiased(self):
            """True when the loaders' resize is the antialiased one: a filter other than "bilinear" and a resize set
            (Resample("bilinear"), or no resize, is as without the option)."""
            return (self._resample is not None and not self._resample.is_bilinear
                    and (self.resize_width > 0 or self.scale is not None))

        def _resampled(self, rgbs):
            """The full-resolution work-dtype images rgbs of one shape resized to the ISP's resize geometry by the
            antialiased resize, in ONE launch.  DESIGN.md 3, "Antialiased resize"."""
            if not rgbs:
                return rgbs
            h, w = rgbs[0].shape[:2]
            hd, wd, scale = self._geometry(h, w)
            outs = [torch.empty((hd, wd, 3), dtype=torch_dtype, device=self.device) for _ in rgbs]
            _rs.apply(rgbs, outs, self._resample.filter, h, w, hd, wd, scale, scale, dtype.code, dtype.code, self.device)
            return outs

        def _check_resample_fits(self, shape):
            """ValueError when the antialiased resize does not take the ISP's scale on a frame of `shape` (before
            anything is uploaded or launched)."""
            if self._antialiased():
                hd, wd, scale = self._geometry(*shape)
                _rs.check_geometry(self._resample.filter, shape[0], shape[1], hd, wd, scale, scale)

        @property
        def local_tonemap(self) -> Optional[_ltm.LocalTonemap]:
            """The LocalTonemap the loaders apply to the images they return, or None."""
            return self._ltm

        def _tone_mapped(self, rgbs):
            """The images of a loader call as the caller gets them: with local tone mapping on, mapped in place by ONE call
            behind everything else of the load on the same stream (the images carry no metering subsample then, so the
            metering and the tonemaps see the mapped image); else as they are.  DESIGN.md 3, "Local tone mapping"."""
            if self._ltm is not None and rgbs:
                _ltm.apply(rgbs, self._ltm)
                _written_in_place(rgbs)
            return rgbs

        @property
        def sharpen(self) -> Optional[_shp.Sharpen]:
            """The Sharpen the tonemaps apply to their u8 outputs, or None."""
            return self._sharpen

        def _sharpened(self, outputs, yuv420=False):
            """The u8 outputs of a tonemap as the caller gets them: with sharpening on, new tensors holding the filter of
            `outputs` (which were then the tonemap's temporaries; one launch behind it on the same stream), else
            `outputs` themselves.  DESIGN.md 3, "Output sharpening"."""
            if self._sharpen is None or not outputs:
                return outputs
            return _shp.apply(outputs, self._sharpen, yuv420)

        @property
        def local_contrast(self) -> Optional[_lc.LocalContrast]:
            """The LocalContrast the tonemaps apply to their u8 outputs, or None."""
            return self._local_contrast

        def _check_local_contrast_fits(self, images):
            """ValueError for an image whose output (after the orientation transform) does not take the tile grid, before a
            tonemap launches anything or moves the metering state."""
            if self._local_contrast is not None:
                for im in images:
                    if isinstance(im, torch.Tensor) and im.ndim >= 2:
                        _lc.check_shape(*_out_shape(im, self.transform)[:2], self._local_contrast)

        @property
        def chroma_denoise(self) -> Optional[_cdn.ChromaDenoise]:
            """The ChromaDenoise the tonemaps apply to their u8 outputs, or None."""
            return self._chroma_denoise

        @property
        def luma_denoise(self) -> Optional[_ydn.LumaDenoise]:
            """The LumaDenoise the tonemaps apply to their u8 outputs, or None."""
            return self._luma_denoise

        @property
        def color_lut(self) -> Optional[_clut.ColorLut]:
            """The ColorLut the tonemaps map their u8 RGB outputs through, or None."""
            return self._color_lut

        def _finished(self, outputs, yuv420=False):
            """The u8 outputs of a tonemap as the caller gets them: the colour LUT, in place on `outputs` (the tonemap's
            own freshly allocated RGB tensors; planar YUV outputs have been through it before their conversion:
            tonemap_reinhard_yuv420), then chroma noise reduction (a stencil: new tensors, which take the place of
            `outputs`), then luma noise reduction (another stencil, likewise), then local contrast, in place on those,
            then sharpening; with none set, `outputs` themselves.  DESIGN.md 3, "Colour LUT", "Chroma noise reduction",
            "Luma noise reduction", "Local contrast" and "Output sharpening"."""
            if self._color_lut is not None and outputs and not yuv420:
                _clut.apply(outputs, self._color_lut, inplace=True)
            if self._chroma_denoise is not None and outputs:
                outputs = _cdn.apply(outputs, self._chroma_denoise, yuv420)
            if self._luma_denoise is not None and outputs:
                outputs = _ydn.apply(outputs, self._luma_denoise, yuv420)
            if self._local_contrast is not None and outputs:
                _lc.apply(outputs, self._local_contrast, yuv420, inplace=True)
            return self._sharpened(outputs, yuv420)

        @property
        def lens_shading(self) -> Optional[torch.Tensor]:
            """The lens shading grid the loaders apply, (sites, Gh, Gw) f32 on the device (do not write it; use set), or
            None."""
            return self._shading

        def _levels(self, bits):
            """The Levels argument of the *_levels entry points for a `bits`-bit source, None without levels (ValueError
            for levels that do not fit it - raised before anything is launched)."""
            lv = _check_levels(self.black_level, self.white_level, bits)
            return None if lv is None else _native.levels_arg(*lv)

        def _geometry(self, h, w):
            """(hd, wd, scale) of resize_image's output for an h x w frame (camera_isp.py:302-312), scale 0.0 without a
            resize."""
            if self.resize_width > 0:
                scale = self.resize_width / w
                return round(h * scale), self.resize_width, scale
            if self.scale is not None:
                return round(h * self.scale), round(w * self.scale), self.scale
            return h, w, 0.0

        def resize_image(self, image):
            """camera_isp.py:302-315."""
            if self.resize_width <= 0 and self.scale is None:
                return image
            hd, wd, scale = self._geometry(*image.shape[:2])
            if self._antialiased():
                return interpolate.resample(image, (wd, hd), scale, self._resample.filter)
            return interpolate.resize_bilinear(image, (wd, hd), scale)

        def _convert(self, image, mode, src_dtype, defects=None, undistort=None, history=None):
            if not isinstance(image, torch.Tensor):
                raise TypeError("image must be a torch.Tensor")
            assert image.ndim == 2, "image must be a 2-D CFA"
            assert image.dtype == src_dtype, f"image must be {src_dtype}, got {image.dtype}"
            self._merge_state(False, ("load_16u", "load_32f", "load_16f")[mode])
            h, w = image.shape
            dm = _defects.check_defects(defects, (h, w))
            lens = self._check_lens(undistort, (h, w))
            lv = self._levels(16)
            if lv is not None and mode != 0:
                raise ValueError("black_level / white_level apply to raw codes (load_16u, load_packed12/16); "
                                 "load_16f / load_32f take normalised values")
            if self._chromatic is not None:
                self._chromatic.check_shape((h, w))      # (before anything is uploaded or launched)
            hists = _tn.check_histories(self._temporal, None if history is None else [history], 1, (h, w), self.device)
            self._check_resample_fits((h, w))
            self._check_statistics_fits((h, w))
            L = _native.lib()
            stream = _native.stream_ptr(self.device)
            src = image.to(self.device).contiguous()
            if self._raw_stage_on():                     # the raw stages that are on: one launch each
                cfa = self._raw_chain([src], h, w, _native.MI_RAW_16U + mode, False, lv, [dm], hists)[0]
            else:
                cfa = torch.empty((h, w), dtype=torch_dtype, device=self.device)
                # (NULL levels and a NULL grid are exactly the plain mi_isp_load_convert, include/mi_isp.h)
                _native.check(L.mi_isp_load_convert_shading(src.data_ptr(), cfa.data_ptr(), h, w, mode, dtype.code, lv,
                                                            _native.shading_arg(self._applied_shading()), stream))
                if dm is not None:                       # defective pixels: the CFA's listed sites, in place
                    _native.check(L.mi_isp_defects_fix_cfa(cfa.data_ptr(), h, w, dtype.code, dm._arg(self.device), stream))
            self._awb_stats_cfa(src, h, w, mode, lv)     # auto white balance: the statistics of the source
            self._frame_stats([src], h, w, _native.MI_RAW_16U + mode, False, lv, [dm])
            return self._tone_mapped([self._process_image(cfa, lens)])[0]

        def load_16u(self, image, defects=None, undistort=None, history=None):
            """camera_isp.py:318-321 (kernel :82-87).  defects (an extension): None or the DefectMap of this sensor.
            undistort (an extension): None or the lens.LensDistortion of this camera ("Lens distortion").
            history (an extension): with temporal_denoise on, the TemporalHistory of this camera ("Temporal
            noise reduction"); None otherwise."""
            return self._convert(image, 0, torch.uint16, defects, undistort, history)

        def load_16f(self, image, defects=None, undistort=None, history=None):
            """camera_isp.py:323-326 (kernel :95-99: u16 converted numerically)."""
            return self._convert(image, 2, torch.uint16, defects, undistort, history)

        def load_32f(self, image, defects=None, undistort=None, history=None):
            """camera_isp.py:328-331 (kernel :89-93)."""
            return self._convert(image, 1, torch.float32, defects, undistort, history)

        def _check_lens(self, undistort, shape):
            """The lens of a frame of `shape` (None: none); ValueError for another frame shape or a table of another
            output shape than the loader's."""
            if undistort is None:
                return None
            if self._antialiased():
                # the remap runs at the frame's own size and scale 1, and the antialiased resize follows
                if undistort.is_table and tuple(undistort.table_shape) != tuple(shape):
                    raise ValueError(f"with resample={self._resample.filter!r} the lens remap runs at the frame's own "
                                     f"size before the resize: a lens table must have the frame's shape {tuple(shape)}, "
                                     f"got {tuple(undistort.table_shape)}")
                return _lens.check_lens(undistort, shape, tuple(shape))
            return _lens.check_lens(undistort, shape, self._geometry(*shape)[:2])

        def _undistort(self, rgbs, lenses, h, w, full=False):
            """The full-resolution work-dtype images rgbs remapped through lenses (one each, none None) into new images
            at the ISP's resize geometry, at scale 1 without a resize (one launch for the analytic lenses).  With the
            antialiased resize the remap runs at the frame's own size and scale 1 and the resize follows; full: the
            caller resizes (all images of its call in one launch)."""
            hd, wd, scale = (h, w, 0.0) if self._antialiased() else self._geometry(h, w)
            scale = scale or 1.0                         # (no resize: the remap at scale 1)
            outs = [torch.empty((hd, wd, 3), dtype=torch_dtype, device=self.device) for _ in rgbs]
            if hd * wd:
                _lens.apply(lenses, rgbs, outs, h, w, hd, wd, scale, scale, dtype.code, dtype.code, self.device)
            # (the antialiased resize: the remap above ran at the frame's own size and scale 1, the resize follows)
            return self._resampled(outs) if self._antialiased() and not full else outs

        def _fix_defects(self, srcs, rgbs, subs, maps, h, w, bits, ids_format, hd, wd, scale, lv, sh):
            """The sparse fix-up after a packed load on the same stream: every output pixel of rgbs[i] (and its metering
            subsample entry) that reads a site of maps[i] (None: none) recomputed from the packed frame; one launch."""
            L = _native.lib()
            stream = _native.stream_ptr(self.device)
            ccm = _native.ccm_arg(self.color_correct_matrix)
            st = self.metering_stride if subs is not None else 1
            lists = [None if m is None else m._outputs(self.device, hd, wd, scale) for m in maps]
            if len(srcs) == 1:
                if lists[0][1] == 0:
                    return
                _native.check(L.mi_isp_defects_fix_packed(
                    srcs[0].data_ptr(), rgbs[0].data_ptr(), h, w, bits, int(bool(ids_format)), self._demosaic_pattern.value,
                    ccm, dtype.code, hd, wd, float(scale), None if subs is None else subs[0].data_ptr(), st, lv, sh,
                    maps[0]._arg(self.device), lists[0][0].data_ptr(), lists[0][1], stream))
                return
            args, p_maps = self._map_args(maps)
            p_lists = (ctypes.c_void_p * len(maps))(*[None if l is None else l[0].data_ptr() for l in lists])
            counts = (ctypes.c_int32 * len(maps))(*[0 if l is None else l[1] for l in lists])
            _native.check(L.mi_isp_defects_fix_packed_batch(
                _native.ptr_array(srcs), _native.ptr_array(rgbs), None if subs is None else _native.ptr_array(subs),
                len(srcs), h, w, bits, int(bool(ids_format)), self._demosaic_pattern.value, ccm, dtype.code, hd, wd,
                float(scale), st, lv, sh, p_maps, p_lists, counts, stream))

        @staticmethod
        def _packed_shape(frames, bits):
            """(h, w) of the packed frames of one call (camera_isp.py:336,343), checked: (H, bytes) uint8 tensors of one
            shape that hold whole pixels of an even-size image."""
            f0 = frames[0]
            for d in frames:
                if not isinstance(d, torch.Tensor):
                    raise TypeError("image_data must be a torch.Tensor")
                assert d.ndim == 2 and d.dtype == torch.uint8, "image_data must be (H, bytes) uint8"
                assert d is f0 or d.shape == f0.shape, "the frames of a batch must share a shape"
            h, row = f0.shape
            if bits == 12:
                assert row % 3 == 0, "packed-12 rows must hold whole pixel pairs (bytes % 3 == 0)"
            w = row * 2 // 3 if bits == 12 else row // 2
            assert w % 2 == 0 and h % 2 == 0, "image must be even size"
            return h, w

        @staticmethod
        def _per_frame(what, values, n, shape, check):
            """The per-frame entries of a defects= / undistort= argument, each through check(entry, shape): None for a
            frame without one, all None for None; ValueError for anything but a list of n entries."""
            if values is None:
                return [None] * n
            if not isinstance(values, (list, tuple)):
                raise ValueError(f"{what} must be None or a list with one entry per frame, got {type(values).__name__}")
            if len(values) != n:
                raise ValueError(f"{what} has {len(values)} entries for {n} frames")
            return [check(v, shape) for v in values]

        def _load_packed(self, frames, bits, ids_format, defects, undistort, batch, history=None):
            """Every packed loader: the frames checked (levels, defect maps and lenses too, before anything is uploaded or
            launched), loaded by their route - raw noise reduction, lens remap, or the plain load - and, with auto white
            balance on, their statistics added to the pending sums in one launch behind the loads.  defects, undistort:
            None or one entry per frame; history: with temporal noise reduction on, one TemporalHistory per frame.  batch:
            the caller is the batch surface (see _load_frames)."""
            self._merge_state(False, f"load_packed{bits}")
            h, w = self._packed_shape(frames, bits)
            lv = self._levels(bits)
            maps = self._per_frame("defects", defects, len(frames), (h, w), _defects.check_defects)
            lenses = self._per_frame("undistort", undistort, len(frames), (h, w), self._check_lens)
            if self._chromatic is not None:
                self._chromatic.check_shape((h, w))
            if history is not None and not isinstance(history, (list, tuple)):
                raise ValueError(f"history must be None or a list with one TemporalHistory per frame, got "
                                 f"{type(history).__name__}")
            hists = _tn.check_histories(self._temporal, history, len(frames), (h, w), self.device)
            self._check_resample_fits((h, w))
            self._check_statistics_fits((h, w))
            srcs = [d.to(self.device).contiguous() for d in frames]
            aa = self._antialiased()                     # (every route below then stays at full resolution)
            if self._raw_stage_on():
                # the raw stages - highlight reconstruction, chromatic aberration, temporal noise reduction, raw noise
                # reduction - that are on: one launch each, then per frame
                kind = _native.MI_RAW_PACKED12 if bits == 12 else _native.MI_RAW_PACKED16
                cfas = self._raw_chain(srcs, h, w, kind, ids_format, lv, maps, hists)
                rgbs = [(self._process_full if aa else self._process_image)(c, m) for c, m in zip(cfas, lenses)]
            elif self._directional():
                rgbs = self._load_directional(srcs, h, w, bits, ids_format, lv, maps, lenses, keep_size=aa)
            elif aa:
                # the antialiased resize: the frames loaded at full resolution in one launch, without the fused resize and
                # the fused metering subsample, the defect fix-up on those images, then each lens remap at the frame's size
                rgbs = self._load_frames(srcs, h, w, bits, ids_format, lv, maps, True, full=True)
                rest = [i for i, m in enumerate(lenses) if m is not None]
                if rest:
                    for i, out in zip(rest, self._undistort([rgbs[i] for i in rest], [lenses[i] for i in rest], h, w,
                                                            full=True)):
                        rgbs[i] = out
            elif lenses.count(None) < len(lenses):       # (some frame has a lens)
                # lens distortion: the frames without a lens as the call without lenses, the others loaded at full
                # resolution in one launch and remapped
                plain = [i for i, m in enumerate(lenses) if m is None]
                rest = [i for i, m in enumerate(lenses) if m is not None]
                out = dict(zip(plain, self._load_frames([srcs[i] for i in plain], h, w, bits, ids_format, lv,
                                                        [maps[i] for i in plain], batch) if plain else []))
                full = self._load_frames([srcs[i] for i in rest], h, w, bits, ids_format, lv, [maps[i] for i in rest],
                                         True, full=True)
                out.update(zip(rest, self._undistort(full, [lenses[i] for i in rest], h, w)))
                rgbs = [out[i] for i in range(len(srcs))]
            else:
                rgbs = self._load_frames(srcs, h, w, bits, ids_format, lv, maps, batch)
            if aa:
                rgbs = self._resampled(rgbs)             # (all images of the call in ONE launch)
            self._awb_stats_packed(srcs, h, w, bits, ids_format, lv)     # auto white balance: the statistics of the sources
            self._frame_stats(srcs, h, w, _native.MI_RAW_PACKED12 if bits == 12 else _native.MI_RAW_PACKED16, ids_format, lv,
                              maps)
            return self._tone_mapped(rgbs)

        def _load_directional(self, srcs, h, w, bits, ids_format, lv, maps, lenses, keep_size=False):
            """The packed loaders' route with the directional demosaic and no raw stage on: the frames without a defect map
            go from packed bytes to the full-resolution image in ONE launch (mi_isp_demosaic_directional_raw_batch: the
            CFA exists in LDS only); a frame with a map is decoded to its CFA (one launch for all of them), fixed in place
            and demosaiced from there.  Then each image is resized, or remapped through its lens, as _process_image does:
            the fused resize and the fused metering subsample are not used.  DESIGN.md 3, "Directional demosaic"."""
            L = _native.lib()
            stream = _native.stream_ptr(self.device)
            kind = _native.MI_RAW_PACKED12 if bits == 12 else _native.MI_RAW_PACKED16
            ids = int(bool(ids_format))
            sh = _native.shading_arg(self._applied_shading())
            plain = [i for i, m in enumerate(maps) if m is None]
            mapped = [i for i, m in enumerate(maps) if m is not None]
            out = {}
            if plain:
                full = [torch.empty((h, w, 3), dtype=torch_dtype, device=self.device) for _ in plain]
                _native.check(L.mi_isp_demosaic_directional_raw_batch(
                    _native.ptr_array([srcs[i] for i in plain]), _native.ptr_array(full), len(plain), h, w, kind, ids,
                    dtype.code, self._demosaic_pattern.value, lv, sh, _native.ccm_arg(self.color_correct_matrix), stream))
                for i, rgb in zip(plain, full):
                    if lenses[i] is not None:
                        out[i] = self._undistort([rgb], [lenses[i]], h, w, full=keep_size)[0]
                    else:
                        out[i] = rgb if keep_size else self.resize_image(rgb)
            if mapped:
                cfas = [torch.empty((h, w), dtype=torch_dtype, device=self.device) for _ in mapped]
                _native.check(L.mi_isp_raw_cfa_batch(_native.ptr_array([srcs[i] for i in mapped]), _native.ptr_array(cfas),
                                                     len(mapped), h, w, kind, ids, dtype.code, lv, sh, stream))
                for i, cfa in zip(mapped, cfas):
                    _native.check(L.mi_isp_defects_fix_cfa(cfa.data_ptr(), h, w, dtype.code, maps[i]._arg(self.device),
                                                           stream))
                    out[i] = (self._process_full if keep_size else self._process_image)(cfa, lenses[i])
            return [out[i] for i in range(len(srcs))]

        def _load_frames(self, srcs, h, w, bits, ids_format, lv, maps, batch, full=False):
            """The load itself: the checked h x w packed frames srcs (on the device; maps: a DefectMap or None each) to
            new work-dtype images at the resize geometry, then the defect fix-up on the same stream.  batch selects only
            the entry point that launches: the batch surface loads all frames in one launch of the batch entry point, the
            single-frame surface its one frame through the single-frame ones.  full: at full resolution whatever the
            resize settings and without a metering subsample (the source of a lens remap).
            The library's *_shading entry points take levels and a grid that may each be NULL; NULL / NULL is exactly the
            plain call (include/mi_isp.h)."""
            L = _native.lib()
            ids, st = int(bool(ids_format)), self.metering_stride
            hd, wd, scale = (h, w, 0.0) if full else self._geometry(h, w)
            fused = scale > 0 and min(hd, wd) > 0 and L.mi_isp_load_packed_scale_supported(float(scale))
            separate = scale > 0 and not fused           # a scale the fused kernel does not take: resize separately
            if separate and batch:                       # (frame by frame through the single-frame route)
                return [self._load_frames([s], h, w, bits, ids_format, lv, [m], False)[0] for s, m in zip(srcs, maps)]
            if not fused:
                hd, wd, scale = h, w, 0.0
            # the image and, on the way, the stride-subsampled copy update_metering will ask for (camera_isp.py:168-170):
            # the load kernel holds those pixels anyway, the strided gather over six 4K images costs 25 us per call
            # (local tone mapping rewrites the image behind the load: no subsample of the unmapped one)
            metered = not (full or fused or separate) and self._ltm is None and bool(
                L.mi_isp_load_packed_metered_is_fused(h, w, bits, ids, dtype.code, st))
            rgbs = [torch.empty((hd, wd, 3), dtype=torch_dtype, device=self.device) for _ in srcs]
            subs = [torch.empty(((hd + st - 1) // st, (wd + st - 1) // st, 3), dtype=torch_dtype, device=self.device)
                    for _ in srcs] if metered else None
            sh = _native.shading_arg(self._applied_shading())
            frame = (h, w, bits, ids, self._demosaic_pattern.value, _native.ccm_arg(self.color_correct_matrix), dtype.code,
                     hd, wd, float(scale))
            stream = _native.stream_ptr(self.device)
            if batch:
                _native.check(L.mi_isp_load_packed_batch_shading(
                    _native.ptr_array(srcs), _native.ptr_array(rgbs), None if subs is None else _native.ptr_array(subs),
                    len(srcs), *frame, st, lv, sh, stream))
            elif metered:
                _native.check(L.mi_isp_load_packed_metered_shading(srcs[0].data_ptr(), rgbs[0].data_ptr(), *frame,
                                                                   subs[0].data_ptr(), st, lv, sh, stream))
            else:
                _native.check(L.mi_isp_load_packed_shading(srcs[0].data_ptr(), rgbs[0].data_ptr(), *frame, lv, sh, stream))
            if maps.count(None) < len(maps):             # (some frame has a map)
                self._fix_defects(srcs, rgbs, subs, maps, h, w, bits, ids_format, hd, wd, float(scale), lv, sh)
            if metered:
                for rgb, sub in zip(rgbs, subs):
                    _tag_subsample(rgb, sub, st)
            return [self.resize_image(rgb) for rgb in rgbs] if separate else rgbs

        def load_packed12(self, image_data, ids_format=False, defects=None, undistort=None, history=None):
            """camera_isp.py:333-340: unpack + demosaic (+ccm) fused in one pass over the packed frame.
            defects (an extension): None or the DefectMap of this sensor ("Defective pixels").
            undistort (an extension): None or the lens.LensDistortion of this camera ("Lens distortion"): the
            frame is loaded at full resolution, then remapped at the resize geometry (the fused resize is not used).
            history (an extension): with temporal_denoise on, the TemporalHistory of this camera: the frame is filtered
            against it and becomes its new content ("Temporal noise reduction"); None otherwise."""
            return self._load_packed([image_data], 12, ids_format, None if defects is None else [defects],
                                     None if undistort is None else [undistort], False,
                                     None if history is None else [history])[0]

        def load_packed16(self, image_data, defects=None, undistort=None, history=None):
            """camera_isp.py:342-347."""
            return self._load_packed([image_data], 16, False, None if defects is None else [defects],
                                     None if undistort is None else [undistort], False,
                                     None if history is None else [history])[0]

        def load_packed12_batch(self, images_data: List[torch.Tensor], ids_format=False,
                                defects=None, undistort=None, history=None) -> List[torch.Tensor]:
            """Extension (not in the reference): `[self.load_packed12(d, ids_format) for d in images_data]` for the cameras
            of one group - frames of one size - in ONE launch per 8 cameras (mi_isp_load_packed_batch): same results, bit
            for bit, without the other launches' dispatch, table build and drain (config 3: 43.0 -> 39.5 us per frame).
            defects: None, or one entry per frame (a DefectMap or None); the fix-ups of all frames take one launch.
            undistort: None, or one entry per frame (a LensDistortion or None); the analytic remaps take one launch.
            history: with temporal_denoise on, a list with the TemporalHistory of each frame's camera (no object twice);
            the frames' temporal stage takes one launch."""
            _typecheck("images_data", images_data, list)
            if not images_data:
                _tn.check_histories(self._temporal, history, 0, (0, 0), self.device)
                self.frame_statistics = None if self._statistics is None else []
                return []
            return self._load_packed(images_data, 12, ids_format, defects, undistort, True, history)

        def load_packed16_batch(self, images_data: List[torch.Tensor], defects=None,
                                undistort=None, history=None) -> List[torch.Tensor]:
            """The same for `load_packed16` (camera_isp.py:342-347)."""
            _typecheck("images_data", images_data, list)
            if not images_data:
                _tn.check_histories(self._temporal, history, 0, (0, 0), self.device)
                self.frame_statistics = None if self._statistics is None else []
                return []
            return self._load_packed(images_data, 16, False, defects, undistort, True, history)

        def _convert_bracket(self, frames, mode, src_dtype, defects=None, undistort=None, history=None):
            """The bracket form of _convert: the E frames of one bracket (exposure merge on), merged and taken through
            the raw stages that are on; everything is checked before anything is uploaded or launched."""
            what = ("load_16u_bracket", "load_32f_bracket", "load_16f_bracket")[mode]
            self._merge_state(True, what)
            frames = _em.check_bracket(frames, self._merge)
            assert frames[0].ndim == 2, "the frames must be 2-D CFAs"
            assert frames[0].dtype == src_dtype, f"the frames must be {src_dtype}, got {frames[0].dtype}"
            h, w = frames[0].shape
            dm = _defects.check_defects(defects, (h, w))
            lens = self._check_lens(undistort, (h, w))
            lv = self._levels(16)
            if lv is not None and mode != 0:
                raise ValueError("black_level / white_level apply to raw codes (load_16u, load_packed12/16); "
                                 "load_16f / load_32f take normalised values")
            if self._chromatic is not None:
                self._chromatic.check_shape((h, w))
            self._check_statistics_fits((h, w))
            hists = _tn.check_histories(self._temporal, None if history is None else [history], 1, (h, w), self.device)
            srcs = [f.to(self.device).contiguous() for f in frames]
            cfa = self._raw_chain([srcs[0]], h, w, _native.MI_RAW_16U + mode, False, lv, [dm], hists, brackets=[srcs])[0]
            self._awb_stats_cfa(srcs[0], h, w, mode, lv)   # auto white balance: the statistics of frame 0 (the output's units)
            self._frame_stats(srcs, h, w, _native.MI_RAW_16U + mode, False, lv, [dm], exposures=len(srcs))
            return self._tone_mapped([self._process_image(cfa, lens)])[0]

        def load_16u_bracket(self, frames, defects=None, undistort=None, history=None):
            """Extension: `load_16u` of an exposure bracket (exposure_merge on): frames holds the E frames of one camera
            and one instant, the shortest exposure first; they are merged into one linear raw frame in the units of the
            shortest ("Exposure merge"), which then takes the raw stages that are on.  defects: the one
            DefectMap of the sensor; history: with temporal_denoise on, the TemporalHistory of this camera."""
            return self._convert_bracket(frames, 0, torch.uint16, defects, undistort, history)

        def load_16f_bracket(self, frames, defects=None, undistort=None, history=None):
            """The same for `load_16f`."""
            return self._convert_bracket(frames, 2, torch.uint16, defects, undistort, history)

        def load_32f_bracket(self, frames, defects=None, undistort=None, history=None):
            """The same for `load_32f`."""
            return self._convert_bracket(frames, 1, torch.float32, defects, undistort, history)

        def _load_packed_brackets(self, brackets, bits, ids_format, defects, undistort, history):
            """Every packed bracket loader: the brackets checked (levels, defect maps, lenses and histories too, before
            anything is uploaded or launched), merged in ONE launch and taken through the raw stages that are on; with auto
            white balance on the statistics of every bracket's frame 0 are added to the pending sums.  defects, undistort,
            history: None or one entry per bracket."""
            what = f"load_packed{bits}_bracket"
            self._merge_state(True, what)
            if not isinstance(brackets, (list, tuple)):
                raise ValueError(f"{what}: brackets must be a list of brackets, got {type(brackets).__name__}")
            brackets = [_em.check_bracket(b, self._merge, f"bracket {i}") for i, b in enumerate(brackets)]
            n = len(brackets)
            if history is not None and not isinstance(history, (list, tuple)):
                raise ValueError(f"history must be None or a list with one TemporalHistory per bracket, got "
                                 f"{type(history).__name__}")
            if n == 0:
                _tn.check_histories(self._temporal, history, 0, (0, 0), self.device)
                self.frame_statistics = None if self._statistics is None else []
                return []
            f0 = brackets[0][0]
            for i, b in enumerate(brackets):
                if b[0].shape != f0.shape or b[0].dtype != f0.dtype:
                    raise ValueError(f"bracket {i} holds {tuple(b[0].shape)} {b[0].dtype} frames, bracket 0 "
                                     f"{tuple(f0.shape)} {f0.dtype}: the brackets of a call share a shape")
            h, w = self._packed_shape([f for b in brackets for f in b], bits)
            lv = self._levels(bits)
            maps = self._per_frame("defects", defects, n, (h, w), _defects.check_defects)
            lenses = self._per_frame("undistort", undistort, n, (h, w), self._check_lens)
            if self._chromatic is not None:
                self._chromatic.check_shape((h, w))
            hists = _tn.check_histories(self._temporal, history, n, (h, w), self.device)
            self._check_resample_fits((h, w))
            self._check_statistics_fits((h, w))
            srcs = [[f.to(self.device).contiguous() for f in b] for b in brackets]
            first = [b[0] for b in srcs]
            kind = _native.MI_RAW_PACKED12 if bits == 12 else _native.MI_RAW_PACKED16
            cfas = self._raw_chain(first, h, w, kind, ids_format, lv, maps, hists, brackets=srcs)
            aa = self._antialiased()                     # (the images stay at full resolution, one resize launch for all)
            rgbs = [(self._process_full if aa else self._process_image)(c, m) for c, m in zip(cfas, lenses)]
            if aa:
                rgbs = self._resampled(rgbs)
            self._awb_stats_packed(first, h, w, bits, ids_format, lv)    # auto white balance: each bracket's frame 0
            self._frame_stats([f for b in srcs for f in b], h, w, kind, ids_format, lv, maps, exposures=len(srcs[0]))
            return self._tone_mapped(rgbs)

        def load_packed12_bracket(self, frames, ids_format=False, defects=None, undistort=None, history=None):
            """Extension: `load_packed12` of an exposure bracket (exposure_merge on): frames holds the E packed frames of
            one camera and one instant, the shortest exposure first ("Exposure merge").  defects: the one
            DefectMap of the sensor; history: with temporal_denoise on, the TemporalHistory of this camera, which then
            holds the merged frame."""
            self._merge_state(True, "load_packed12_bracket")
            return self._load_packed_brackets([frames], 12, ids_format, None if defects is None else [defects],
                                              None if undistort is None else [undistort],
                                              None if history is None else [history])[0]

        def load_packed16_bracket(self, frames, defects=None, undistort=None, history=None):
            """The same for `load_packed16`."""
            self._merge_state(True, "load_packed16_bracket")
            return self._load_packed_brackets([frames], 16, False, None if defects is None else [defects],
                                              None if undistort is None else [undistort],
                                              None if history is None else [history])[0]

        def load_packed12_bracket_batch(self, brackets, ids_format=False, defects=None, undistort=None,
                                        history=None) -> List[torch.Tensor]:
            """`[self.load_packed12_bracket(b, ids_format) for b in brackets]` for the cameras of one group - brackets of
            one size - with ONE merge launch per 16 brackets: same results, bit for bit.  defects, undistort, history: None,
            or one entry per bracket."""
            return self._load_packed_brackets(brackets, 12, ids_format, defects, undistort, history)

        def load_packed16_bracket_batch(self, brackets, defects=None, undistort=None, history=None) -> List[torch.Tensor]:
            """The same for `load_packed16_bracket`."""
            return self._load_packed_brackets(brackets, 16, False, defects, undistort, history)

        @property
        def color_correct_matrix(self) -> Optional[np.ndarray]:
            """camera_isp.py:360-369: cc with column j scaled by white_balance[j].  With auto white balance on, cc as it
            is: the AWB gains are applied in the raw domain instead."""
            if self.correct_colors:
                cc = self.color_correction.copy()
                if self._awb is None:
                    cc[:, :3] *= self.white_balance
                return cc
            return None

        def _demosaiced(self, cfa):
            demosaic = _dm.directional if self._directional() else bayer.bayer_to_rgb
            return demosaic(cfa, pattern=self._demosaic_pattern, correct_colors=self.color_correct_matrix)

        def _process_image(self, cfa, lens=None):
            """camera_isp.py:371-373; with a lens the full-resolution image is remapped at the resize geometry."""
            rgb = self._demosaiced(cfa)
            if lens is not None:
                return self._undistort([rgb], [lens], *cfa.shape)[0]
            return self.resize_image(rgb)

        def _process_full(self, cfa, lens=None):
            """_process_image without the resize (the antialiased resize: the caller resizes all images of its call in one
            launch); a lens remaps at the frame's own size."""
            rgb = self._demosaiced(cfa)
            return rgb if lens is None else self._undistort([rgb], [lens], *cfa.shape, full=True)[0]

        def _metering_images(self, images, t, prev, stride=None):
            """camera_isp.py:168-175: statistics of the stride-subsampled images, blended into a
            copy of `prev`; the subsample is gathered in-kernel (no torch.stack copy)."""
            assert len(images) > 0, "need at least one image"
            for im in images:
                _check_image(im)
                assert im.shape == images[0].shape, "all images of one call must share a shape"
            H, W = images[0].shape[:2]
            ws = _native.workspace(H, W, self.device)
            stride = self.metering_stride if stride is None else stride       # (stride=1: the caller hands over subsamples)
            # images that came out of load_packed12 / 16 carry their subsample: the same samples in the same order from a
            # dense buffer (stride 1) - identical results, no strided gather over the full-size images
            subs = [_valid_subsample(im, stride) for im in images]
            if all(s is not None for s in subs):
                images = subs
                H, W = images[0].shape[:2]
                stride = 1
            ptrs = _native.ptr_array(images)
            L = _native.lib()
            stream = _native.stream_ptr(self.device)
            _raise_resident_faults(L, self.device)
            if self.process_group is None:
                # (the reference clones `prev` and lets the kernel update the clone, camera_isp.py:172-173; here the kernel
                # reads `prev` and writes the new tensor: no copy kernel - 4 us - in front of every update)
                metering = torch.empty_like(prev)
                _native.check(L.mi_isp_metering_to(ptrs, len(images), H, W, stride, dtype.code, prev.data_ptr(),
                                                   metering.data_ptr(), float(t), ws.data_ptr(), stream))
                return metering
            # sharded batch: the same two data passes, an all-gather after each (two collectives per call), the ranks'
            # rows combined by one small kernel each on this stream (mi_isp_metering_combine_*)
            world = _dist.world_size(self.process_group)
            raw = torch.empty(2, dtype=torch.float32, device=self.device)
            _native.check(L.mi_isp_metering_bounds(ptrs, len(images), H, W, stride, dtype.code,
                                                   raw.data_ptr(), ws.data_ptr(), stream))
            gathered = _dist.all_gather_rows(raw, self.process_group)
            b = torch.empty(2, dtype=torch.float32, device=self.device)
            _native.check(L.mi_isp_metering_combine_bounds(gathered.data_ptr(), world, prev.data_ptr(), float(t),
                                                           b.data_ptr(), stream))
            part = torch.empty(8, dtype=torch.float32, device=self.device)
            _native.check(L.mi_isp_metering_sums(ptrs, len(images), H, W, stride, dtype.code,
                                                 b.data_ptr(), part.data_ptr(), ws.data_ptr(), stream))
            gathered8 = _dist.all_gather_rows(part, self.process_group)
            metering = prev.clone()
            _native.check(L.mi_isp_metering_combine_sums(gathered8.data_ptr(), world, b.data_ptr(), metering.data_ptr(),
                                                         float(t), stream))
            return metering

        def update_metering(self, images: List[torch.Tensor]):
            """camera_isp.py:376-385."""
            if self.metrics is None:
                initial = torch.zeros(9, dtype=torch.float32, device=self.device)
                self.metrics = self._metering_images(images, 0.0, initial)
            else:
                self.metrics = self._metering_images(images, (1.0 - self.moving_alpha), self.metrics)
            self.update_white_balance()                  # (auto white balance: a no-op when off)

        def tonemap_only(self, image, metrics, gamma, intensity, light_adapt, color_adapt):
            """camera_isp.py:387-390."""
            self._check_local_contrast_fits([image])
            output = torch.empty(_out_shape(image, self.transform), dtype=torch.uint8, device=self.device)
            reinhard_kernel(image, output, metrics, gamma, intensity, light_adapt, color_adapt, self.transform)
            return self._finished([output])[0]

        def tonemap_reinhard(self, images: List[torch.Tensor],
                             gamma: float = 1.0, intensity: float = 1.0, light_adapt: float = 1.0,
                             color_adapt: float = 0.0, write_back: bool = True):
            """camera_isp.py:394-403.  NOTE: like the reference, pass 1 overwrites each input image
            with the Reinhard-mapped values (camera_isp.py:211).
            write_back=False (an extension, not the reference's semantics): the same u8 outputs, bit for bit, with the
            images left as they are - a third of the tonemap's memory traffic is that write and its re-read."""
            _typecheck("images", images, list)
            self._check_local_contrast_fits(images)
            return self._finished(self._tonemap_reinhard(images, gamma, intensity, light_adapt, color_adapt, write_back))

        def _tonemap_reinhard(self, images, gamma, intensity, light_adapt, color_adapt, write_back=True):
            """tonemap_reinhard before local contrast and output sharpening."""
            _typecheck("write_back", write_back, bool)
            _typecheck("images", images, list)
            for n, v in (("gamma", gamma), ("intensity", intensity), ("light_adapt", light_adapt),
                         ("color_adapt", color_adapt)):
                _typecheck(n, v, float)
            _check_transform(images, self.transform)
            self.update_metering(images)
            outputs = [torch.empty(_out_shape(image, self.transform), dtype=torch.uint8, device=self.device)
                       for image in images]
            # one batched call for the whole list (the reference loops, camera_isp.py:400-401); the
            # orientation transform (:403) is folded into the u8 store
            H, W = images[0].shape[:2]
            ws = _native.workspace(H, W, self.device)
            fn = _native.lib().mi_isp_reinhard_batch if write_back else _native.lib().mi_isp_reinhard_batch_keep
            _native.check(fn(
                _native.ptr_array(images), _native.ptr_array(outputs), len(images), H, W, dtype.code,
                self.metrics.data_ptr(), float(gamma), float(intensity), float(light_adapt), float(color_adapt),
                interpolate.transform_code(self.transform), ws.data_ptr(), _native.stream_ptr(self.device)))
            if write_back:
                _written_in_place(images)
            return outputs

        def tonemap_reinhard_yuv420(self, images: List[torch.Tensor],
                                    gamma: float = 1.0, intensity: float = 1.0, light_adapt: float = 1.0,
                                    color_adapt: float = 0.0):
            """Extension (not in the reference): `[color.rgb_yuv420_image(o) for o in tonemap_reinhard(images, ...)]`
            - planar YUV 4:2:0 u8 `(H * 3 / 2, W)` per image for video encoders - with the conversion
            (color/yuv_420.py:39-66) fused into the second Reinhard pass when no orientation transform is set
            and W % 16 == 0: the u8 RGB images are never written.  Same side effects as tonemap_reinhard.
            With sharpen= set, the Y plane of each YUV image is sharpened (sharpen.unsharp_mask_yuv420), which is not the
            YUV image of a sharpened RGB output; local_contrast= likewise equalises the Y plane
            (local_contrast.clahe_yuv420), and chroma_denoise= filters the U and V planes
            (chroma_denoise.chroma_denoise_yuv420) and luma_denoise= the Y plane (luma_denoise.luma_denoise_yuv420), before
            both.  A 3D LUT has no planar form: with color_lut= set the RGB
            outputs are written, mapped through the table and converted (the unfused branch), then the planar operators
            run."""
            from . import color
            _typecheck("images", images, list)
            self._check_local_contrast_fits(images)
            H, W = images[0].shape[:2]
            if self.transform != interpolate.ImageTransform.none or H % 2 or W % 16 or self._color_lut is not None:
                rgb = self._tonemap_reinhard(images, gamma, intensity, light_adapt, color_adapt)
                if self._color_lut is not None and rgb:
                    _clut.apply(rgb, self._color_lut, inplace=True)
                return self._finished([color.rgb_yuv420_image(o) for o in rgb], yuv420=True)
            for n, v in (("gamma", gamma), ("intensity", intensity), ("light_adapt", light_adapt),
                         ("color_adapt", color_adapt)):
                _typecheck(n, v, float)
            self.update_metering(images)
            outputs = [torch.empty((H * 3 // 2, W), dtype=torch.uint8, device=self.device) for _ in images]
            ws = _native.workspace(H, W, self.device)
            _native.check(_native.lib().mi_isp_reinhard_batch_yuv420(
                _native.ptr_array(images), _native.ptr_array(outputs), len(images), H, W, dtype.code,
                self.metrics.data_ptr(), float(gamma), float(intensity), float(light_adapt), float(color_adapt),
                ws.data_ptr(), _native.stream_ptr(self.device)))
            _written_in_place(images)
            return self._finished(outputs, yuv420=True)

        def process_packed12(self, frames: List[torch.Tensor], gamma: float = 1.0, intensity: float = 1.0,
                             light_adapt: float = 1.0, color_adapt: float = 0.0, keep_images: bool = False,
                             ids_format: bool = False, defects=None, undistort=None, history=None):
            """Extension (not in the reference): one step of the reference's own bench in one call -
            `Processor.__call__` of bench/camera_isp.py:23-27:

                images = [isp.load_packed12(f, ids_format) for f in frames]
                return isp.tonemap_reinhard(images, gamma=...)

            with the same u8 outputs and the same metering state afterwards, bit for bit.  For a full-resolution
            Camera16 group that fits the chip (`mi_isp_camera_group_fits`: 4096 x 3072 on MI355X, metering stride 8, no
            resize, no orientation transform, no lens shading grid, no auto white balance, single process, every packed frame 4-byte aligned) the
            loaded images never exist in memory: the metering reads a subsample demosaiced straight from the packed frames, and ONE persistent
            launch takes every camera from packed bytes to its u8 image (csrc/isp_mega_cam.h).  Everything else takes the
            two calls above.
            keep_images=True returns `(outputs, images)`, the images holding what the reference leaves in them (p,
            camera_isp.py:211); by default only the outputs are returned, as the bench's Processor does.
            local_tonemap= on always takes the two calls.
            defects: None, or one entry per frame (a DefectMap or None); any map takes the two calls, the load with
            `defects=`.  undistort: the same for lenses (a LensDistortion or None per frame).  history: with
            temporal_denoise on (always the two calls), one TemporalHistory per frame."""
            _typecheck("frames", frames, list)
            _typecheck("keep_images", keep_images, bool)
            for n, v in (("gamma", gamma), ("intensity", intensity), ("light_adapt", light_adapt),
                         ("color_adapt", color_adapt)):
                _typecheck(n, v, float)
            assert len(frames) > 0, "need at least one frame"
            self._merge_state(False, "process_packed12")
            L = _native.lib()
            f0 = frames[0]
            lv = self._levels(12)                            # (sensor levels: checked before anything runs)
            if defects is not None or undistort is not None:     # (defect maps and lenses too)
                shape = self._packed_shape(frames, 12)
                maps = self._per_frame("defects", defects, len(frames), shape, _defects.check_defects)
                lenses = self._per_frame("undistort", undistort, len(frames), shape, self._check_lens)
                defects = maps if any(m is not None for m in maps) else None
                undistort = lenses if any(m is not None for m in lenses) else None

            def group(name, *args, tail=()):
                """The camera-group entry point `name`; with levels its _levels twin, which takes them ahead of `tail`."""
                if lv is None:
                    return getattr(L, name)(*args, *tail)
                return getattr(L, name + "_levels")(*args, lv, *tail)

            fused = (dtype is types.f16 and not ids_format and self.resize_width == 0 and self.scale is None
                     and self._applied_shading() is None      # (lens shading or AWB: the two calls below)
                     and self._raw_denoise is None            # (raw noise reduction: the two calls below)
                     and self._highlights is None             # (highlight reconstruction: the two calls below)
                     and self._dynamic_defects is None        # (dynamic defects: the two calls below)
                     and self._green_equalize is None         # (green equalisation: the two calls below)
                     and self._chromatic is None              # (chromatic aberration: the two calls below)
                     and self._temporal is None               # (temporal noise reduction: the two calls below)
                     and self._ltm is None                    # (local tone mapping: the two calls below)
                     and not self._directional()              # (the directional demosaic: the two calls below)
                     and history is None                     # (a history without it: the load below rejects it)
                     and defects is None                      # (defective pixels: the two calls below)
                     and undistort is None                    # (lens distortion: the two calls below)
                     and self.transform == interpolate.ImageTransform.none and self.metering_stride == 8
                     and 1 <= len(frames) <= 64
                     and all(isinstance(f, torch.Tensor) and f.ndim == 2 and f.dtype == torch.uint8 and f.shape == f0.shape
                             for f in frames)
                     and f0.shape[1] % 3 == 0)
            srcs = [f.to(self.device).contiguous() for f in frames] if fused else None
            # (the camera-group kernel reads the packed rows as 4-byte words: a frame that is a view at another byte offset
            # takes the two calls, whose loader reads it byte by byte)
            fused = fused and all(s.data_ptr() % 4 == 0 for s in srcs)
            if fused and torch.cuda.is_current_stream_capturing():
                fused = False                  # (a captured resident launch can be neither ordered against others nor checked)
            if fused:
                h, w = f0.shape[0], f0.shape[1] * 2 // 3
                self._check_statistics_fits((h, w))
                with torch.cuda.device(self.device):
                    fused = bool(group("mi_isp_camera_group_fits", h, w, self._demosaic_pattern.value, dtype.code, 8))
            if not fused:
                images = self.load_packed12_batch(frames, ids_format, defects=defects, undistort=undistort,
                                                  history=history)
                outputs = self.tonemap_reinhard(images, gamma, intensity, light_adapt, color_adapt)
                return (outputs, images) if keep_images else outputs
            if self._local_contrast is not None:
                _lc.check_shape(h, w, self._local_contrast)
            _raise_resident_faults(L, self.device)
            n = len(srcs)
            outputs = [torch.empty((h, w, 3), dtype=torch.uint8, device=self.device) for _ in srcs]
            images = [torch.empty((h, w, 3), dtype=torch_dtype, device=self.device) for _ in srcs] if keep_images else None
            if self.metrics is None:                         # camera_isp.py:376-385
                prev, t = torch.zeros(9, dtype=torch.float32, device=self.device), 0.0
            else:
                prev, t = self.metrics, 1.0 - self.moving_alpha
            metrics = torch.empty_like(prev)                 # (the previous state is read, the new one written: no clone)
            scratch = torch.empty(int(L.mi_isp_camera_group_scratch_bytes(n, h, w)), dtype=torch.uint8, device=self.device)
            ws = _native.workspace(h, w, self.device, slots=n + 1)
            stream = _native.stream_ptr(self.device)
            p_srcs, p_imgs, p_outs = _native.ptr_array(srcs), _native.ptr_array(images) if keep_images else None, _native.ptr_array(outputs)
            ccm = _native.ccm_arg(self.color_correct_matrix)
            if self.process_group is None:
                args = (p_srcs, p_imgs, p_outs, n, h, w, self._demosaic_pattern.value, ccm, prev.data_ptr(), metrics.data_ptr(),
                        float(t), float(gamma), float(intensity), float(light_adapt), float(color_adapt), scratch.data_ptr(),
                        ws.data_ptr())
                _native.check(group("mi_isp_camera_group_reinhard", *args, tail=(stream,)))
                self.metrics = metrics
                self._frame_stats(srcs, h, w, _native.MI_RAW_PACKED12, False, lv, [None] * n)
                outputs = self._finished(outputs)
                return (outputs, images) if keep_images else outputs
            # a sharded group (one process per GPU): the same three steps with the metering's two all-gathers in between
            _native.check(group("mi_isp_camera_group_subsample", p_srcs, n, h, w, self._demosaic_pattern.value, ccm,
                                scratch.data_ptr(), tail=(stream,)))
            per = int(L.mi_isp_camera_group_scratch_bytes(1, h, w))
            hs, ws_ = (h + 7) // 8, (w + 7) // 8
            subs = [scratch[i * per:i * per + hs * ws_ * 6].view(torch_dtype).view(hs, ws_, 3) for i in range(n)]
            self.metrics = self._metering_images(subs, t, prev, stride=1)
            args = (p_srcs, p_imgs, p_outs, n, h, w, self._demosaic_pattern.value, ccm, self.metrics.data_ptr(), float(gamma),
                    float(intensity), float(light_adapt), float(color_adapt), ws.data_ptr())
            _native.check(group("mi_isp_camera_group_tonemap", *args, tail=(stream,)))
            self._frame_stats(srcs, h, w, _native.MI_RAW_PACKED12, False, lv, [None] * n)
            outputs = self._finished(outputs)
            return (outputs, images) if keep_images else outputs

        def tonemap_linear(self, images: List[torch.Tensor], gamma: float = 1.0):
            """camera_isp.py:405-413."""
            _typecheck("images", images, list)
            _typecheck("gamma", gamma, float)
            _check_transform(images, self.transform)
            self._check_local_contrast_fits(images)
            self.update_metering(images)
            outputs = [torch.empty(_out_shape(image, self.transform), dtype=torch.uint8, device=self.device)
                       for image in images]
            H, W = images[0].shape[:2]
            ws = _native.workspace(H, W, self.device)
            _native.check(_native.lib().mi_isp_linear_batch(
                _native.ptr_array(images), _native.ptr_array(outputs), len(images), H, W, dtype.code,
                self.metrics.data_ptr(), float(gamma), interpolate.transform_code(self.transform), ws.data_ptr(),
                _native.stream_ptr(self.device)))
            return self._finished(outputs)

    ISP.reinhard_kernel = staticmethod(reinhard_kernel)
    ISP.linear_kernel = staticmethod(linear_kernel)
    ISP.dtype = dtype
    ISP.__name__ = name
    ISP.__qualname__ = name
    return ISP


Camera16 = camera_isp("Camera16", types.f16)
Camera32 = camera_isp("Camera32", types.f32)
