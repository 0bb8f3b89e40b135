"""ctypes binding of libmi355_isp.so (include/mi_isp.h) and device-buffer plumbing.

PyTorch-ROCm tensors are only the device-buffer / stream provider here.  There is no CPU
fallback: every public op raises if the HIP library or a GPU is missing.
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p, POINTER

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI_ISP_LIB: an instrumented build of the same library (measurement only, e.g. scripts/tile_stamps.py)
LIB_PATH = os.environ.get("MI_ISP_LIB") or os.path.join(_HERE, "lib", "libmi355_isp.so")

MI_U8, MI_U16, MI_F16, MI_F32 = 0, 1, 2, 3
# source kinds of mi_isp_denoise_raw(_batch)
MI_RAW_PACKED12, MI_RAW_PACKED16, MI_RAW_16U, MI_RAW_32F, MI_RAW_16F = 0, 1, 2, 3, 4


class Levels(ctypes.Structure):
    """mi_isp_levels: the sensor's black level per CFA site ((row & 1) * 2 + (col & 1)) and its white level."""
    _fields_ = [("black", c_int32 * 4), ("white", c_int32)]


class Shading(ctypes.Structure):
    """mi_isp_shading: a lens shading gain grid on the device, `sites` (1 or 4) x grid_h x grid_w f32."""
    _fields_ = [("gains_dev", c_void_p), ("sites", c_int32), ("grid_h", c_int32), ("grid_w", c_int32)]


class Defects(ctypes.Structure):
    """mi_isp_defects: a defect map on the device, n (row, col) int32 pairs and a bit mask of H rows x ceil(W / 32) u32."""
    _fields_ = [("coords_dev", c_void_p), ("n", c_int32), ("mask_dev", c_void_p)]


class Lens(ctypes.Structure):
    """mi_isp_lens: K, new_K, up to 8 distortion coefficients in OpenCV order (k1, k2, p1, p2, k3, k4, k5, k6), how many
    of them (4, 5 or 8) and the border mode (MI_BORDER_CONSTANT 0, MI_BORDER_REPLICATE 1)."""
    _fields_ = [("fx", c_double), ("fy", c_double), ("cx", c_double), ("cy", c_double),
                ("new_fx", c_double), ("new_fy", c_double), ("new_cx", c_double), ("new_cy", c_double),
                ("dist", c_double * 8), ("n_dist", c_int32), ("border", c_int32)]


class Denoise(ctypes.Structure):
    """mi_isp_denoise: the raw noise filter's noise model (gain, read_noise, in the loader's x units), strength,
    spatial_sigma and radius (1 or 2)."""
    _fields_ = [("gain", c_float), ("read_noise", c_float), ("strength", c_float), ("spatial_sigma", c_float),
                ("radius", c_int32)]


class DynamicDefects(ctypes.Structure):
    """mi_isp_dynamic_defects: the threshold and its slope, how many of a pixel's neighbours may be defective themselves
    (0 or 1), and whether hot and dead pixels are looked for."""
    _fields_ = [("threshold", c_float), ("slope", c_float), ("tolerate", c_int32), ("hot", c_int32), ("dead", c_int32)]


class GreenEqualize(ctypes.Structure):
    """mi_isp_green_equalize: the threshold of the believed imbalance and its slope over the signal, the strength of the
    correction, the radius of the local means (1 or 2) and the edge gate's factor."""
    _fields_ = [("threshold", c_float), ("slope", c_float), ("strength", c_float), ("radius", c_int32), ("edge", c_float)]


class Statistics(ctypes.Structure):
    """mi_isp_statistics: the zone grid (rows, columns), the clip level and the dark level."""
    _fields_ = [("zones_h", c_int32), ("zones_w", c_int32), ("clip", c_float), ("dark", c_float)]


class Highlights(ctypes.Structure):
    """mi_isp_highlights: the mode (0 rebuild, 1 clip), the clip level, the balance gains of R, G, B and, when not NULL,
    3 f32 on the device that override them."""
    _fields_ = [("mode", c_int32), ("clip", c_float), ("wb", c_float * 3), ("wb_dev", c_void_p)]


class Chromatic(ctypes.Structure):
    """mi_isp_chromatic: the optical centre (cy, cx) and the normalisation radius in raw pixels, and (k0, k1, k2) of the
    red and of the blue channel's scale."""
    _fields_ = [("cy", c_double), ("cx", c_double), ("norm_radius", c_double), ("red", c_double * 3),
                ("blue", c_double * 3)]


class Sharpen(ctypes.Structure):
    """mi_isp_sharpen: the output sharpening filter's amount times 64 (0 .. 512), radius (1 or 2), coring threshold
    (0 .. 255) and halo clamp overshoot (0 .. 255, -1: none)."""
    _fields_ = [("amount_q6", c_int32), ("radius", c_int32), ("threshold", c_int32), ("overshoot", c_int32)]


class LocalContrast(ctypes.Structure):
    """mi_isp_local_contrast: the tile grid (1 .. 16 each way), the clip limit times 256 (256 .. 16384, 0: no clip) and
    the strength times 64 (0 .. 64)."""
    _fields_ = [("tiles_y", c_int32), ("tiles_x", c_int32), ("clip_q8", c_int32), ("strength_q6", c_int32)]


class LocalTonemap(ctypes.Structure):
    """mi_isp_local_tonemap: the strength (0 .. 1), the white and floor of the log-luminance range, the anchor whose gain is
    1, the cell side in pixels (8, 16, 32 or 64) and the luminance bins (2 .. 32)."""
    _fields_ = [("strength", c_float), ("white", c_float), ("floor", c_float), ("anchor", c_float), ("cell", c_int32),
                ("bins", c_int32)]


class ExposureMerge(ctypes.Structure):
    """mi_isp_exposure_merge: the number of exposures, their ratios (the shortest first, ratio[0] == 1), the noise model
    (gain, read_noise, in the units of the shortest frame's x), the saturation level and knee of the long frames and the
    rejection threshold in noise standard deviations."""
    _fields_ = [("n", c_int32), ("ratio", c_float * 4), ("gain", c_float), ("read_noise", c_float),
                ("saturation", c_float), ("knee", c_float), ("threshold", c_float)]


class Temporal(ctypes.Structure):
    """mi_isp_temporal: the temporal filter's noise model (gain, read_noise, in the loader's x units), the threshold in
    noise standard deviations and the weight of the past on a static pixel."""
    _fields_ = [("gain", c_float), ("read_noise", c_float), ("threshold", c_float), ("max_weight", c_float)]


class ChromaDenoise(ctypes.Structure):
    """mi_isp_chroma_denoise: the window radius in cells (1, 2 or 3), the luma and chroma thresholds (0 .. 255) and the
    strength times 64 (0 .. 64)."""
    _fields_ = [("radius", c_int32), ("luma_threshold", c_int32), ("chroma_threshold", c_int32), ("strength_q6", c_int32)]


class LumaDenoise(ctypes.Structure):
    """mi_isp_luma_denoise: the window radius in pixels (1, 2 or 3), the thresholds in the dark and in the bright (0 .. 255
    luma codes) and the strength times 64 (0 .. 64)."""
    _fields_ = [("radius", c_int32), ("threshold", c_int32), ("threshold_bright", c_int32), ("strength_q6", c_int32)]


class ResampleAxis(ctypes.Structure):
    """mi_isp_resample_axis: the table of one axis of the antialiased resize: its taps, and the starts (D int32) and the
    weights (D x taps f32) on the device."""
    _fields_ = [("taps", c_int32), ("start_dev", c_void_p), ("weight_dev", c_void_p)]


class ColorLut(ctypes.Structure):
    """mi_isp_color_lut: the table's points per axis (2 .. 65) and the strength times 64 (0 .. 64)."""
    _fields_ = [("n_points", c_int32), ("strength_q6", c_int32)]


class Route(ctypes.Structure):
    """mi_isp_route: the chain mi_isp_pipeline12_reinhard takes (ROUTES), the tile first pass's HOT specialisation, the
    streaming kernels' rows per wave and column bands (0 on the tile routes), the first pass's blocks."""
    _fields_ = [("route", c_int32), ("hot", c_int32), ("rows_per_wave", c_int32), ("bands_x", c_int32), ("n_blocks", c_int32)]


# MI_ISP_ROUTE_*
ROUTES = ("stream", "cached_stream", "cached_tile", "recompute")


# every symbol include/mi_isp.h declares: name -> (restype, argtypes)
_P = c_void_p
SIGNATURES = {
    "mi_isp_version": (c_int, []),
    "mi_isp_last_error": (c_char_p, []),
    "mi_isp_bayer_weights": (c_int, [POINTER(c_int32)]),
    "mi_isp_workspace_bytes": (c_size_t, [c_int, c_int]),
    "mi_isp_decode12": (c_int, [_P, _P, c_int64, c_int, c_int, c_int, _P]),
    "mi_isp_decode16": (c_int, [_P, _P, c_int64, c_int, c_int, _P]),
    "mi_isp_encode12": (c_int, [_P, _P, c_int64, c_int, c_int, c_int, _P]),
    "mi_isp_load_convert": (c_int, [_P, _P, c_int64, c_int, c_int, _P]),
    "mi_isp_demosaic": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), _P]),
    "mi_isp_mosaic": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "mi_isp_rgb_to_yuv420": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "mi_isp_rgb_to_yuv420_is_vector": (c_int, [_P, _P, c_int, c_int, c_int]),
    "mi_isp_yuv420_to_rgb": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "mi_isp_resize_bilinear": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, _P]),
    "mi_isp_transform": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "mi_isp_metering": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, c_int, _P, c_float, _P, _P]),
    "mi_isp_metering_to": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, c_int, _P, _P, c_float, _P, _P]),
    "mi_isp_metering_bounds": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, c_int, _P, _P, _P]),
    "mi_isp_metering_sums": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P]),
    "mi_isp_reinhard": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_float, c_float, c_float, c_float, c_int, _P, _P]),
    "mi_isp_reinhard_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, _P, c_float, c_float, c_float,
                                      c_float, c_int, _P, _P]),
    "mi_isp_reinhard_batch_keep": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, _P, c_float, c_float, c_float,
                                           c_float, c_int, _P, _P]),
    "mi_isp_reinhard_batch_yuv420": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, _P, c_float, c_float,
                                             c_float, c_float, _P, _P]),
    "mi_isp_linear_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, _P, c_float, c_int, _P, _P]),
    "mi_isp_linear": (c_int, [_P, _P, c_int, c_int, c_int, _P, c_float, c_int, _P, _P]),
    "mi_isp_tonemap_linear": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_float, _P, _P]),
    "mi_isp_tonemap_reinhard": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_float, _P, _P]),
    "mi_isp_tonemap_pass_geometry": (c_int, [c_int, c_int, c_int, c_int, _P, _P, POINTER(c_int64)]),
    "mi_isp_load_packed": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int, c_int,
                                   c_float, _P]),
    "mi_isp_load_packed_metered": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int, c_int,
                                           c_float, _P, c_int, _P]),
    "mi_isp_load_packed_batch": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int,
                                         POINTER(c_float), c_int, c_int, c_int, c_float, c_int, _P]),
    "mi_isp_load_packed_levels": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int, c_int,
                                          c_float, POINTER(Levels), _P]),
    "mi_isp_load_packed_metered_levels": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int,
                                                  c_int, c_float, _P, c_int, POINTER(Levels), _P]),
    "mi_isp_load_packed_batch_levels": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int,
                                                c_int, POINTER(c_float), c_int, c_int, c_int, c_float, c_int,
                                                POINTER(Levels), _P]),
    "mi_isp_load_convert_levels": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(Levels), _P]),
    "mi_isp_load_packed_shading": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int,
                                           c_int, c_float, POINTER(Levels), POINTER(Shading), _P]),
    "mi_isp_load_packed_metered_shading": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int,
                                                   c_int, c_int, c_float, _P, c_int, POINTER(Levels), POINTER(Shading),
                                                   _P]),
    "mi_isp_load_packed_batch_shading": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int,
                                                 c_int, c_int, POINTER(c_float), c_int, c_int, c_int, c_float, c_int,
                                                 POINTER(Levels), POINTER(Shading), _P]),
    "mi_isp_load_convert_shading": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading), _P]),
    "mi_isp_defects_fix_packed": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int, c_int,
                                          c_float, _P, c_int, POINTER(Levels), POINTER(Shading), POINTER(Defects), _P,
                                          c_int, _P]),
    "mi_isp_defects_fix_packed_batch": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int,
                                                c_int, POINTER(c_float), c_int, c_int, c_int, c_float, c_int,
                                                POINTER(Levels), POINTER(Shading), POINTER(_P), POINTER(_P),
                                                POINTER(c_int32), _P]),
    "mi_isp_defects_fix_cfa": (c_int, [_P, c_int, c_int, c_int, POINTER(Defects), _P]),
    "mi_isp_undistort": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_float, c_float, c_int, c_int, POINTER(Lens), _P]),
    "mi_isp_undistort_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_int,
                                       c_int, POINTER(_P), _P]),
    "mi_isp_remap": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "mi_isp_awb_stats_packed": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                        c_float, c_float, c_int, _P, _P]),
    "mi_isp_awb_stats_cfa": (c_int, [_P, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading), c_float, c_float, c_int,
                                     _P, _P]),
    "mi_isp_awb_update": (c_int, [_P, c_int, _P, c_int, c_double, _P, _P, POINTER(Shading), _P, _P]),
    "mi_isp_awb_rebuild": (c_int, [c_int, _P, POINTER(Shading), _P, _P]),
    "mi_isp_denoise_raw": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                   POINTER(Defects), POINTER(Denoise), _P]),
    "mi_isp_denoise_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int,
                                         POINTER(Levels), POINTER(Shading), POINTER(_P), POINTER(Denoise), _P]),
    "mi_isp_denoise_cfa": (c_int, [_P, _P, c_int, c_int, c_int, POINTER(Denoise), _P]),
    "mi_isp_highlights_raw": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                      POINTER(Defects), POINTER(Highlights), c_int, _P]),
    "mi_isp_highlights_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                            POINTER(Levels), POINTER(Shading), POINTER(_P), POINTER(Highlights), c_int,
                                            _P]),
    "mi_isp_highlights_cfa": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(Highlights), _P]),
    "mi_isp_dynamic_defects_raw": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                           POINTER(Defects), POINTER(DynamicDefects), c_int, _P, _P]),
    "mi_isp_dynamic_defects_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int,
                                                 POINTER(Levels), POINTER(Shading), POINTER(_P), POINTER(DynamicDefects),
                                                 c_int, _P, POINTER(_P)]),
    "mi_isp_dynamic_defects_cfa": (c_int, [_P, _P, c_int, c_int, c_int, POINTER(DynamicDefects), _P, _P]),
    "mi_isp_green_equalize_raw": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                          POINTER(Defects), POINTER(GreenEqualize), c_int, _P]),
    "mi_isp_green_equalize_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                                POINTER(Levels), POINTER(Shading), POINTER(_P), POINTER(GreenEqualize),
                                                c_int, _P]),
    "mi_isp_green_equalize_cfa": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(GreenEqualize), _P]),
    "mi_isp_statistics_words": (c_int64, [POINTER(Statistics)]),
    "mi_isp_statistics_geometry": (c_int, [POINTER(c_int32)]),
    "mi_isp_statistics_strip": (c_int, [c_int, c_int, c_int]),
    "mi_isp_statistics_direct_blocks": (c_int, [c_int, c_int, c_int, POINTER(Statistics)]),
    "mi_isp_statistics_raw": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Defects),
                                      POINTER(Statistics), _P]),
    "mi_isp_statistics_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int,
                                            POINTER(Levels), POINTER(_P), POINTER(Statistics), _P]),
    "mi_isp_statistics_cfa": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(Defects), POINTER(Statistics), _P]),
    "mi_isp_demosaic_directional_cfa": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(c_float), _P]),
    "mi_isp_demosaic_directional_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int,
                                                      c_int, POINTER(Levels), POINTER(Shading), POINTER(c_float), _P]),
    "mi_isp_raw_cfa_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int, POINTER(Levels),
                                     POINTER(Shading), _P]),
    "mi_isp_chromatic_raw": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                     POINTER(Defects), POINTER(Chromatic), c_int, _P]),
    "mi_isp_chromatic_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                           POINTER(Levels), POINTER(Shading), POINTER(_P), POINTER(Chromatic), c_int,
                                           _P]),
    "mi_isp_chromatic_cfa": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(Chromatic), _P]),
    "mi_isp_sharpen_rgb_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(Sharpen), _P]),
    "mi_isp_sharpen_yuv420_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(Sharpen), _P]),
    "mi_isp_local_contrast_workspace_bytes": (c_size_t, [c_int, POINTER(LocalContrast)]),
    "mi_isp_local_contrast_rgb_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(LocalContrast), _P,
                                                _P]),
    "mi_isp_local_contrast_yuv420_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(LocalContrast),
                                                   _P, _P]),
    "mi_isp_temporal_raw": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                    POINTER(Defects), POINTER(Temporal), c_int, _P]),
    "mi_isp_temporal_raw_batch": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int,
                                          c_int, c_int, POINTER(Levels), POINTER(Shading), POINTER(_P), POINTER(Temporal),
                                          c_int, _P]),
    "mi_isp_temporal_cfa": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, POINTER(Temporal), _P]),
    "mi_isp_merge_raw": (c_int, [POINTER(_P), _P, c_int, c_int, c_int, c_int, c_int, POINTER(Levels), POINTER(Shading),
                                 POINTER(Defects), POINTER(ExposureMerge), c_int, _P]),
    "mi_isp_merge_raw_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int, POINTER(Levels),
                                       POINTER(Shading), POINTER(_P), POINTER(ExposureMerge), c_int, _P]),
    "mi_isp_merge_cfa": (c_int, [POINTER(_P), _P, c_int, c_int, c_int, POINTER(ExposureMerge), _P]),
    "mi_isp_local_tonemap_workspace_bytes": (c_size_t, [c_int, c_int, c_int, POINTER(LocalTonemap)]),
    "mi_isp_local_tonemap_batch": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, POINTER(LocalTonemap), _P, _P]),
    "mi_isp_local_tonemap_grids": (c_int, [_P, c_int, c_int, c_int, POINTER(LocalTonemap), _P, _P, _P, _P, _P]),
    "mi_isp_resample_taps": (c_int, [c_int, c_int, c_int, c_double]),
    "mi_isp_resample_table": (c_int, [c_int, c_int, c_int, c_double, _P, _P]),
    "mi_isp_resample_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                      POINTER(ResampleAxis), POINTER(ResampleAxis), _P]),
    "mi_isp_chroma_denoise_rgb_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(ChromaDenoise), _P]),
    "mi_isp_chroma_denoise_yuv420_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(ChromaDenoise),
                                                   _P]),
    "mi_isp_luma_denoise_rgb_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(LumaDenoise), _P]),
    "mi_isp_luma_denoise_yuv420_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, POINTER(LumaDenoise), _P]),
    "mi_isp_color_lut_rgb_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, _P, POINTER(ColorLut), _P]),
    "mi_isp_color_lut_rgb_batch_path": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, _P, POINTER(ColorLut), c_int,
                                                _P]),
    "mi_isp_load_packed_metered_is_fused": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int]),
    "mi_isp_load_packed_scale_supported": (c_int, [c_float]),
    "mi_isp_pipeline12_reinhard": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int,
                                           c_float, c_float, c_float, c_float, _P, _P]),
    "mi_isp_pipeline12_route": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, POINTER(Route)]),
    "mi_isp_pipeline12_reinhard_batch": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int,
                                                 POINTER(c_float), c_int, c_int, c_float, c_float, c_float, c_float,
                                                 _P, POINTER(_P), c_int]),
    "mi_isp_pipeline12_pass": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_int, c_float,
                                       c_float, c_float, c_int, _P, _P]),
    "mi_isp_metering_combine_bounds": (c_int, [_P, c_int, _P, c_float, _P, _P]),
    "mi_isp_metering_combine_sums": (c_int, [_P, c_int, _P, _P, c_float, _P]),
    "mi_isp_camera_frame_batch": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int, c_int,
                                          POINTER(c_float), c_int, c_int, c_int, c_float, c_int, _P, c_float, c_int, c_float,
                                          c_float, c_float, c_float, c_int, _P, _P]),
    "mi_isp_camera_group_reinhard": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, POINTER(c_float),
                                             _P, _P, c_float, c_float, c_float, c_float, c_float, _P, _P, _P]),
    "mi_isp_camera_group_subsample": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, POINTER(c_float), _P, _P]),
    "mi_isp_camera_group_tonemap": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, POINTER(c_float),
                                            _P, c_float, c_float, c_float, c_float, _P, _P]),
    "mi_isp_camera_group_fits": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "mi_isp_camera_group_reinhard_levels": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int,
                                                    POINTER(c_float), _P, _P, c_float, c_float, c_float, c_float, c_float, _P,
                                                    _P, POINTER(Levels), _P]),
    "mi_isp_camera_group_subsample_levels": (c_int, [POINTER(_P), c_int, c_int, c_int, c_int, POINTER(c_float), _P,
                                                     POINTER(Levels), _P]),
    "mi_isp_camera_group_tonemap_levels": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int,
                                                   POINTER(c_float), _P, c_float, c_float, c_float, c_float, _P,
                                                   POINTER(Levels), _P]),
    "mi_isp_camera_group_fits_levels": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(Levels)]),
    "mi_isp_camera_group_scratch_bytes": (ctypes.c_size_t, [c_int, c_int, c_int]),
    "mi_isp_camera_group_faults": (c_int, [c_int]),
    "mi_isp_camera_group_set_poll_limit": (c_int, [ctypes.c_uint]),
    "mi_isp_pipeline12_graph_create": (c_int, [POINTER(_P), POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int,
                                               POINTER(c_float), c_int, c_int, c_float, c_float, c_float, c_float, _P,
                                               c_int, c_int, POINTER(_P)]),
    "mi_isp_pipeline12_graph_launch": (c_int, [_P, _P]),
    "mi_isp_pipeline12_graph_destroy": (c_int, [_P]),
    "mi_isp_pipeline12_reinhard_whole_frame": (c_int, [_P, _P, c_int, c_int, c_int, c_int, POINTER(c_float), c_int, c_float, c_float,
                                               c_float, c_float, _P, _P]),
    "mi_isp_pipeline12_whole_frame_fits": (c_int, [c_int, c_int, c_int]),
    "mi_isp_pipeline12_reinhard_whole_frame_batch": (c_int, [POINTER(_P), POINTER(_P), c_int, c_int, c_int, c_int, c_int,
                                                             POINTER(c_float), c_int, c_float, c_float, c_float, c_float, _P, _P]),
    "mi_isp_workspace_check": (c_int, [_P, c_int, c_int, c_int, POINTER(c_int), POINTER(c_int), _P]),
    "mi_isp_whole_frame_faults": (c_int, [c_int]),
    "mi_isp_whole_frame_set_poll_limit": (c_int, [ctypes.c_uint]),
    "mi_isp_whole_frame_set_sabotage": (c_int, [c_int]),
    "mi_isp_metering_faults": (c_int, [c_int]),
    "mi_isp_metering_set_poll_limit": (c_int, [ctypes.c_uint]),
    "mi_isp_workspace_error_offset": (ctypes.c_size_t, [c_int, c_int]),
    "mi_isp_profile_enable": (c_int, [c_int, c_int]),
    "mi_isp_profile_collect": (c_int, [POINTER(c_float), POINTER(c_int)]),   # float[4]
}

_lib = None
_lock = threading.Lock()


class NativeLibraryError(ImportError):
    pass


def lib() -> ctypes.CDLL:
    """Load the HIP library (once).  Raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise NativeLibraryError(
                        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(or `make -C taichi_image_amd/csrc`).  There is no CPU fallback.")
                L = ctypes.CDLL(LIB_PATH)
                guarded = _GuardedLibrary()
                for name, (res, args) in SIGNATURES.items():
                    fn = getattr(L, name)   # AttributeError if the library lacks a declared symbol
                    fn.restype, fn.argtypes = res, args
                    setattr(guarded, name, _Guarded(fn))
                _lib = guarded
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("libmi355_isp: " + lib().mi_isp_last_error().decode("utf-8", "replace"))


def require_gpu() -> None:
    if not torch.cuda.is_available():
        raise RuntimeError("taichi_image_amd needs an MI355X (HIP) device; there is no CPU fallback")


class _StreamArg(int):
    """A hipStream_t value that remembers which device it belongs to (see _Guarded)."""
    device = None


def stream_ptr(device: torch.device) -> int:
    s = _StreamArg(torch.cuda.current_stream(device).cuda_stream)
    s.device = device
    return s


class _Guarded:
    """A library entry point that launches on the device its stream argument belongs to.

    The C ABI launches on the CURRENT device (a null stream is every device's default stream), while the call surface
    takes `device=` arguments and tensors of any GPU (camera_isp.py:239-251 of the reference does too).  Every wrapper
    passes its stream through stream_ptr(device); when that device is not the current one the call runs under
    torch.cuda.device(device), so pointers, workspace and launch agree."""

    def __init__(self, fn):
        self.fn = fn

    def __call__(self, *args):
        dev = next((a.device for a in args if isinstance(a, _StreamArg)), None)
        if dev is None or dev.type != "cuda" or dev.index is None or dev.index == torch.cuda.current_device():
            return self.fn(*args)
        with torch.cuda.device(dev):
            return self.fn(*args)


class _GuardedLibrary:
    pass


def ccm_arg(correct_colors):
    """3x3 colour matrix (row-major) -> float[9] or NULL (bayer.py:210-211)."""
    if correct_colors is None:
        return None
    m = np.asarray(correct_colors, dtype=np.float64).reshape(-1)
    assert m.size == 9, "colour correction must be a 3x3 matrix"
    return (c_float * 9)(*[float(v) for v in m])


def pipeline12_route(packed_ptr, out_ptr, work_image_ptr, H, W, ids_format, work_code, out_code):
    """mi_isp_pipeline12_route: (route name of ROUTES, the Route) of these arguments of mi_isp_pipeline12_reinhard.
    Addresses as integers (None / 0: no work image); nothing is launched or dereferenced."""
    r = Route()
    check(lib().mi_isp_pipeline12_route(packed_ptr, out_ptr, work_image_ptr or None, int(H), int(W), int(bool(ids_format)),
                                        int(work_code), int(out_code), ctypes.byref(r)))
    return ROUTES[r.route], r


def rgb_to_yuv420_is_vector(rgb_ptr, yuv_ptr, H, W, out_code):
    """mi_isp_rgb_to_yuv420_is_vector: True when mi_isp_rgb_to_yuv420 runs its vector kernel on these arguments.
    Addresses as integers; nothing is launched or dereferenced."""
    rc = lib().mi_isp_rgb_to_yuv420_is_vector(rgb_ptr, yuv_ptr, int(H), int(W), int(out_code))
    if rc < 0:
        check(rc)
    return bool(rc)


def tonemap_pass_geometry(H, W, in_code, out_code, src_ptr, dst_ptr):
    """mi_isp_tonemap_pass_geometry: (blocks of a storing pass, blocks of a reduce pass, FULL groups, general groups) of
    the stateless tonemaps on these arguments.  Addresses as integers; nothing is launched or dereferenced."""
    out = (c_int64 * 4)()
    check(lib().mi_isp_tonemap_pass_geometry(int(H), int(W), int(in_code), int(out_code), src_ptr, dst_ptr, out))
    return tuple(int(v) for v in out)


def levels_arg(black, white):
    """(black[4], white) -> a Levels for the *_levels entry points; None (no levels) stays None."""
    if black is None:
        return None
    return Levels((c_int32 * 4)(*[int(b) for b in black]), int(white))


def shading_arg(grid):
    """A (sites, grid_h, grid_w) f32 device tensor -> a Shading for the *_shading entry points; None stays None."""
    if grid is None:
        return None
    return Shading(grid.data_ptr(), grid.shape[0], grid.shape[1], grid.shape[2])


_ws_cache: dict = {}


def workspace(H: int, W: int, device: torch.device, slots: int = 1) -> torch.Tensor:
    """Scratch buffer for one in-flight call on (device, current stream)."""
    nbytes = int(lib().mi_isp_workspace_bytes(int(H), int(W))) * slots
    key = (device.index or 0, stream_ptr(device), nbytes)
    ws = _ws_cache.get(key)
    if ws is None:
        if len(_ws_cache) > 64:
            _ws_cache.clear()
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)   # arrival counters start at 0
        _ws_cache[key] = ws
    return ws




def ptr_array(tensors):
    arr = (c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr
