"""Tonemap a multi-camera scan of raw packed-12 frames (the command line of the reference's
`scripts/tonemap_scan.py:104-128`, same arguments and defaults) on the MI355X path.

    python -m taichi_image_amd.scripts.tonemap_scan --scan /data/scan_01 --width 4096 --write out/

A scan is a directory of camera directories holding `.raw` / `.tiff` frames; the frames present in EVERY camera are
processed in natural name order: per frame one `Camera32.load_packed12` per camera and one `tonemap_reinhard` over the
camera group (so the rolling metering is shared, camera_isp.py:376-403), the u8 outputs tiled into a grid.
Host side without OpenCV / natsort / tqdm: grids are written as PNG, nothing is displayed.
"""
from __future__ import annotations

import argparse
import json
import re
import struct
import zipfile
import zlib
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, Iterator, List, Sequence

import numpy as np
import torch

RAW_SUFFIXES = (".raw", ".tiff")
_DIGITS = re.compile(r"(\d+)")


def natural_key(name) -> list:
    """Sort key under which 'img10' follows 'img9' (digit runs compare as numbers, the rest case-insensitively)."""
    return [(0, int(tok)) if tok.isdigit() else (1, tok.lower()) for tok in _DIGITS.split(str(name)) if tok != ""]


@dataclass
class ScanIndex:
    """Which frames to process and where each camera keeps them."""
    cameras: List[Path]                                   # camera directories, natural order
    frames: List[str] = field(default_factory=list)       # file names present in every camera, natural order

    @staticmethod
    def _raw_names(directory: Path) -> set:
        return {e.name for e in directory.iterdir() if e.is_file() and e.suffix in RAW_SUFFIXES}

    @classmethod
    def of_directory(cls, directory) -> "ScanIndex":
        """A single camera: every raw frame of one directory (--images)."""
        directory = Path(directory)
        if not directory.is_dir():
            raise FileNotFoundError(f"Folder {directory} does not exist or is not a directory")
        return cls([directory], sorted(cls._raw_names(directory), key=natural_key))

    @classmethod
    def of_scan(cls, scan_dir) -> "ScanIndex":
        """Every sub-directory with raw frames is a camera; only frames that all cameras have are kept (--scan)."""
        scan_dir = Path(scan_dir)
        if not scan_dir.is_dir():
            raise FileNotFoundError(f"Folder {scan_dir} does not exist or is not a directory")
        per_camera: Dict[Path, set] = {}
        for sub in scan_dir.iterdir():
            if sub.is_dir():
                names = cls._raw_names(sub)
                if names:
                    per_camera[sub] = names
        if not per_camera:
            raise ValueError(f"No image folders found in {scan_dir}")
        shared = set.intersection(*per_camera.values())
        cameras = sorted(per_camera, key=lambda d: natural_key(d.name))
        if not shared:
            raise ValueError(f"No common images found in {[c.name for c in cameras]}")
        return cls(cameras, sorted(shared, key=natural_key))

    def groups(self, loader, reverse: bool = False) -> Iterator:
        """(frame name, [one loaded frame per camera]) with the next group's files already loading (ingest)."""
        from .. import ingest
        names = list(reversed(self.frames)) if reverse else self.frames
        if not names:
            return
        for name, by_camera in ingest.load_images_iter(loader, self.cameras, names):
            yield name, [by_camera[c] for c in self.cameras]


def tile_grid(images: Sequence[torch.Tensor], rows: int) -> torch.Tensor:
    """Images of equal size tiled row-major into `rows` rows (the last row may be shorter only if it is the only one)."""
    per_row = -(-len(images) // max(1, rows))
    strips = [torch.cat(list(images[i:i + per_row]), dim=1) for i in range(0, len(images), per_row)]
    return torch.cat(strips, dim=0)


def write_png(path, image: np.ndarray) -> None:
    """8-bit RGB PNG with the standard library only (the reference writes JPEG through OpenCV)."""
    assert image.ndim == 3 and image.shape[2] == 3 and image.dtype == np.uint8
    h, w, _ = image.shape
    scanlines = np.concatenate([np.zeros((h, 1), np.uint8), image.reshape(h, w * 3)], axis=1).tobytes()   # filter type 0

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(scanlines, 3)) + chunk(b"IEND", b""))


def load_defect_pixels(directory, cameras: Sequence[Path], width: int) -> Dict[str, np.ndarray]:
    """--defect-pixels: `directory/<camera folder name>.npy` holds one camera's (N, 2) integer (row, col) defect
    coordinates; a camera without a file gets no correction.  Checked before any frame is read: ValueError for a file of
    another shape or dtype, a coordinate outside the frame width, or a file that names no camera of the scan (the rows
    are checked against the frame height when the first frame is read)."""
    directory = Path(directory)
    if not directory.is_dir():
        raise FileNotFoundError(f"--defect-pixels: {directory} does not exist or is not a directory")
    names = {c.name for c in cameras}
    maps = {}
    for f in sorted(directory.glob("*.npy"), key=lambda p: natural_key(p.name)):
        if f.stem not in names:
            raise ValueError(f"--defect-pixels: {f.name} names no camera of the scan ({sorted(names)})")
        c = np.load(f, allow_pickle=False)
        if c.size == 0:
            c = np.zeros((0, 2), np.int64)
        if c.ndim != 2 or c.shape[1] != 2 or c.dtype == np.bool_ or not np.issubdtype(c.dtype, np.integer):
            raise ValueError(f"--defect-pixels: {f.name} must hold (N, 2) integer (row, col), got {c.dtype} {c.shape}")
        if len(c) and (c.min() < 0 or c[:, 1].max() >= width):
            raise ValueError(f"--defect-pixels: {f.name} has a coordinate outside a frame {width} pixels wide")
        maps[f.stem] = c
    return maps


def load_lens_distortion(directory, cameras: Sequence[Path]) -> Dict[str, dict]:
    """--lens-distortion: `directory/<camera folder name>.npz` holds one camera's calibration: `K` (3 x 3), `dist` (4, 5 or
    8 coefficients in OpenCV order) and optionally `new_K`; a camera without a file is not undistorted.  Checked before any
    frame is read: ValueError for a file that is no such archive, holds other arrays or invalid values, or names no camera
    of the scan.  Returns the keyword arguments of lens.LensDistortion per camera (the frame shape is added once known)."""
    from ..lens import LensDistortion
    directory = Path(directory)
    if not directory.is_dir():
        raise FileNotFoundError(f"--lens-distortion: {directory} does not exist or is not a directory")
    names = {c.name for c in cameras}
    lenses = {}
    for f in sorted(directory.iterdir(), key=lambda p: natural_key(p.name)):
        if f.suffix != ".npz":
            continue
        if f.stem not in names:
            raise ValueError(f"--lens-distortion: {f.name} names no camera of the scan ({sorted(names)})")
        try:
            with np.load(f, allow_pickle=False) as z:
                arrays = {k: z[k] for k in z.files}
        except (OSError, ValueError, zipfile.BadZipFile) as e:
            raise ValueError(f"--lens-distortion: {f.name} is not a readable .npz archive ({e})") from None
        if not {"K", "dist"} <= set(arrays) or not set(arrays) <= {"K", "dist", "new_K"}:
            raise ValueError(f"--lens-distortion: {f.name} must hold K, dist and optionally new_K, got {sorted(arrays)}")
        kw = {"K": arrays["K"], "dist": arrays["dist"], "new_K": arrays.get("new_K")}
        try:
            LensDistortion(shape=(2, 2), **kw)                         # (the calibration's own checks)
        except ValueError as e:
            raise ValueError(f"--lens-distortion: {f.name}: {e}") from None
        lenses[f.stem] = kw
    return lenses


def statistics_report(settings, cameras, measured):
    """The content of <name>.stats.json: per camera the per-zone means, clipped and dark fractions (zone rows x zone
    columns x the four CFA sites), the sharpness per zone and the 1 / 50 / 99 % percentiles per site; NaN (an empty zone,
    a zone without a focus pixel) is written as null."""
    def plain(a):
        return [plain(v) for v in a] if isinstance(a, list) else (None if a != a else a)
    return {"zones": list(settings.zones), "clip": settings.clip, "dark": settings.dark,
            "cameras": {name: {"mean": plain(m.mean().tolist()), "clipped_fraction": plain(m.clipped_fraction().tolist()),
                               "dark_fraction": plain(m.dark_fraction().tolist()), "sharpness": plain(m.sharpness().tolist()),
                               "percentiles": {str(q): plain([m.percentile(q, site) for site in range(4)]) for q in (1, 50, 99)}}
                        for name, m in zip(cameras, measured)}}


def build_parser() -> argparse.ArgumentParser:
    """The argument surface of scripts/tonemap_scan.py:104-128 (+ --device, --ids_format)."""
    from ..interpolate import ImageTransform

    def transform(s):
        return ImageTransform[s] if s in ImageTransform.__members__ else ImageTransform(s)

    ap = argparse.ArgumentParser(description="Tonemap a scan of raw packed-12 camera frames on an MI355X")
    src = ap.add_argument_group("input")
    src.add_argument("--scan", type=Path)
    src.add_argument("--images", type=Path)
    src.add_argument("--reverse", action="store_true")
    src.add_argument("--width", type=int, default=4096)
    src.add_argument("--ids_format", action="store_true")
    tone = ap.add_argument_group("tonemap")
    tone.add_argument("--gamma", type=float, default=0.9)
    tone.add_argument("--intensity", type=float, default=3.0)
    tone.add_argument("--color_adapt", type=float, default=0.0)
    tone.add_argument("--light_adapt", type=float, default=0.9)
    tone.add_argument("--moving_alpha", type=float, default=0.02)
    tone.add_argument("--resize_width", type=int, default=0)
    tone.add_argument("--transform", type=transform, default=ImageTransform.rotate_90)
    tone.add_argument("--correct_colors", action="store_true")
    # sensor levels (an extension): one black level, or four - one per CFA site (row & 1) * 2 + (col & 1) - and the white
    # level (default: 4095, the packed-12 full scale)
    tone.add_argument("--black-level", dest="black_level", type=int, nargs="+", default=None)
    tone.add_argument("--white-level", dest="white_level", type=int, default=None)
    # lens shading (an extension): a (Gh, Gw) or (4, Gh, Gw) f32 gain grid saved with numpy.save
    # (camera_isp.lens_shading_from_flat makes one from a flat-field capture)
    tone.add_argument("--lens-shading", dest="lens_shading", type=Path, default=None)
    # defective pixels (an extension): a directory of <camera folder name>.npy files, (N, 2) int (row, col) each
    # (defects.find_defects makes one from dark or flat frames)
    tone.add_argument("--defect-pixels", dest="defect_pixels", type=Path, default=None)
    # lens distortion (an extension): a directory of <camera folder name>.npz files holding K, dist (OpenCV order) and
    # optionally new_K
    tone.add_argument("--lens-distortion", dest="lens_distortion", type=Path, default=None)
    # auto white balance (an extension): a gray-world loop over every camera's frames, seeded with the fixed white balance
    tone.add_argument("--auto-white-balance", dest="auto_white_balance", action="store_true")
    # raw noise reduction (an extension): the sensor's noise model, GAIN and READ_NOISE in units of the white level
    # (denoise.noise_model_from_frames fits them from a few frames of a static scene), the filter strength and radius
    tone.add_argument("--raw-denoise", dest="raw_denoise", type=float, nargs=2, metavar=("GAIN", "READ_NOISE"), default=None)
    tone.add_argument("--denoise-strength", dest="denoise_strength", type=float, default=1.0)
    tone.add_argument("--denoise-radius", dest="denoise_radius", type=int, default=1)
    # highlight reconstruction (an extension): clipped raw pixels rebuilt from their neighbours ("rebuild") or every pixel
    # limited to the balanced clip level ("clip"); T the clip level in units of the white level (default 0.98)
    tone.add_argument("--highlights", dest="highlights", choices=("rebuild", "clip"), default=None)
    tone.add_argument("--highlights-clip", dest="highlights_clip", type=float, metavar="T", default=None)
    # dynamic defects (an extension): defective raw pixels found on the fly, without a map, and replaced from their
    # same-site neighbours; T the threshold in units of the white level (default 0.02), S its slope over the signal
    # (default 0.2), K in {0, 1} how many of a pixel's neighbours may be defective themselves (default 1)
    tone.add_argument("--dynamic-defects", dest="dynamic_defects", action="store_true")
    tone.add_argument("--dynamic-defects-threshold", dest="dynamic_defects_threshold", type=float, metavar="T", default=None)
    tone.add_argument("--dynamic-defects-slope", dest="dynamic_defects_slope", type=float, metavar="S", default=None)
    tone.add_argument("--dynamic-defects-tolerate", dest="dynamic_defects_tolerate", type=int, metavar="K", default=None)
    # green equalisation (an extension): the imbalance between the two green sites of a Bayer quad removed in front of the
    # demosaic; T the believed imbalance in units of the white level (default 1/256), S its slope over the signal (default
    # 1/16), A the strength in [0, 1] (default 1), R in {1, 2} the radius of the local means (default 1), E the edge
    # gate's factor (default 4)
    tone.add_argument("--green-equalize", dest="green_equalize", action="store_true")
    tone.add_argument("--green-equalize-threshold", dest="green_equalize_threshold", type=float, metavar="T", default=None)
    tone.add_argument("--green-equalize-slope", dest="green_equalize_slope", type=float, metavar="S", default=None)
    tone.add_argument("--green-equalize-strength", dest="green_equalize_strength", type=float, metavar="A", default=None)
    tone.add_argument("--green-equalize-radius", dest="green_equalize_radius", type=int, metavar="R", default=None)
    tone.add_argument("--green-equalize-edge", dest="green_equalize_edge", type=float, metavar="E", default=None)
    # frame statistics (an extension): the exposure and focus measurements of every raw frame over GH x GW zones, written
    # as <name>.stats.json next to each output (--write)
    tone.add_argument("--statistics", dest="statistics", type=str, metavar="GHxGW", default=None)
    # the demosaic (an extension): "directional" interpolates along edges instead of across them; "malvar" (the default)
    # is the 13-tap filter
    tone.add_argument("--demosaic", dest="demosaic", choices=("malvar", "directional"), default=None)
    # the resize of --resize-width (an extension): "area", "triangle" and "lanczos3" widen with the downscale, so the
    # resized images do not alias; "bilinear" (the default) is the point-sampled resize
    tone.add_argument("--resample", dest="resample", choices=("bilinear", "area", "triangle", "lanczos3"), default=None)
    # chromatic aberration (an extension): (k0, k1, k2) of the red and of the blue channel's radial scale, the optical
    # centre (default: the middle of the frame) and the normalisation radius (default: the half diagonal), in raw pixels
    tone.add_argument("--chromatic-aberration", dest="chromatic_aberration", type=float, nargs=6,
                      metavar=("R0", "R1", "R2", "B0", "B1", "B2"), default=None)
    tone.add_argument("--chromatic-center", dest="chromatic_center", type=float, nargs=2, metavar=("CY", "CX"), default=None)
    tone.add_argument("--chromatic-norm-radius", dest="chromatic_norm_radius", type=float, metavar="R", default=None)
    # temporal noise reduction (an extension): the sensor's noise model as for --raw-denoise, the mean absolute frame
    # difference (in noise standard deviations) at which the past is dropped, and the weight of the past on a static pixel;
    # one history per camera folder, kept across the scan's frames (with --reverse too: it is still a sequence)
    tone.add_argument("--temporal-denoise", dest="temporal_denoise", type=float, nargs=2, metavar=("GAIN", "READ_NOISE"),
                      default=None)
    tone.add_argument("--temporal-threshold", dest="temporal_threshold", type=float, metavar="SIGMAS", default=None)
    tone.add_argument("--temporal-max-weight", dest="temporal_max_weight", type=float, metavar="W", default=None)
    # local tone mapping (an extension): the loaded linear images times an edge-aware local gain (bilateral grid), in front of
    # the global curve; STRENGTH 0 .. 1, the luminance floor of the logarithm (default 2^-10) and the cell side in pixels
    tone.add_argument("--local-tonemap", dest="local_tonemap", type=float, metavar="STRENGTH", default=None)
    tone.add_argument("--local-tonemap-floor", dest="local_tonemap_floor", type=float, metavar="FLOOR", default=None)
    tone.add_argument("--local-tonemap-cell", dest="local_tonemap_cell", type=int, metavar="PIXELS", default=None)
    # output sharpening (an extension): an unsharp mask on the luma of the u8 outputs; AMOUNT 0 .. 8, the blur radius (1 or
    # 2), the coring threshold in luma codes and the halo clamp (luma codes; default: none)
    tone.add_argument("--sharpen", dest="sharpen", type=float, metavar="AMOUNT", default=None)
    tone.add_argument("--sharpen-radius", dest="sharpen_radius", type=int, default=1)
    tone.add_argument("--sharpen-threshold", dest="sharpen_threshold", type=int, default=0)
    tone.add_argument("--sharpen-overshoot", dest="sharpen_overshoot", type=int, default=None)
    # local contrast (an extension): CLAHE on the luma of the u8 outputs, before sharpening; STRENGTH 0 .. 1, the tile grid
    # (rows, columns of the written image) and the clip limit (1 .. 64; 0: no clip)
    tone.add_argument("--local-contrast", dest="local_contrast", type=float, metavar="STRENGTH", default=None)
    tone.add_argument("--local-contrast-tiles", dest="local_contrast_tiles", type=int, nargs=2, metavar=("TY", "TX"),
                      default=None)
    tone.add_argument("--local-contrast-clip", dest="local_contrast_clip", type=float, default=None)
    # chroma noise reduction (an extension): a luma-guided mean of the chroma of the u8 outputs, before local contrast and
    # sharpening; STRENGTH 0 .. 1, the window radius in 2 x 2 pixel cells (1, 2 or 3) and the luma and chroma thresholds
    tone.add_argument("--chroma-denoise", dest="chroma_denoise", type=float, metavar="STRENGTH", default=None)
    tone.add_argument("--chroma-denoise-radius", dest="chroma_denoise_radius", type=int, default=None)
    tone.add_argument("--chroma-denoise-thresholds", dest="chroma_denoise_thresholds", type=int, nargs=2,
                      metavar=("LUMA", "CHROMA"), default=None)
    # luma noise reduction (an extension): an edge-preserving mean of the luma of the u8 outputs, behind chroma noise
    # reduction and before local contrast and sharpening; STRENGTH 0 .. 1, the window radius in pixels (1, 2 or 3) and the
    # thresholds in the dark and in the bright (luma codes)
    tone.add_argument("--luma-denoise", dest="luma_denoise", type=float, metavar="STRENGTH", default=None)
    tone.add_argument("--luma-denoise-radius", dest="luma_denoise_radius", type=int, default=None)
    tone.add_argument("--luma-denoise-thresholds", dest="luma_denoise_thresholds", type=int, nargs=2,
                      metavar=("DARK", "BRIGHT"), default=None)
    # 3D colour LUT (an extension): a .cube file every u8 output is mapped through (tetrahedral interpolation), before the
    # other output operators; STRENGTH 0 .. 1 blends between the input and the table's colour
    tone.add_argument("--color-lut", dest="color_lut", type=Path, metavar="FILE.cube", default=None)
    tone.add_argument("--color-lut-strength", dest="color_lut_strength", type=float, metavar="STRENGTH", default=None)
    out = ap.add_argument_group("output")
    out.add_argument("--write", type=Path, default=None)
    out.add_argument("--rows", type=int, default=2)
    out.add_argument("--device", default="cuda:0")
    return ap


def main(argv=None) -> int:
    from functools import partial
    from .. import bayer, camera_isp, ingest
    from ..defects import DefectMap
    from ..lens import LensDistortion
    from ..denoise import RawDenoise
    from ..highlights import Highlights
    from ..dynamic_defects import DynamicDefects
    from ..green_equalize import GreenEqualize
    from ..statistics import Statistics
    from ..demosaic import Demosaic
    from ..resample import Resample
    from ..chromatic import ChromaticAberration
    from ..temporal import TemporalDenoise, TemporalHistory
    from ..local_tonemap import LocalTonemap
    from ..sharpen import Sharpen
    from ..local_contrast import LocalContrast
    from ..chroma_denoise import ChromaDenoise
    from ..luma_denoise import LumaDenoise
    from ..color_lut import ColorLut
    args = build_parser().parse_args(argv)
    if args.scan is None and args.images is None:
        raise ValueError("No --scan or --images specified")
    black = args.black_level
    if black is not None and len(black) not in (1, 4):
        raise ValueError(f"--black-level takes one value or four (one per CFA site), got {len(black)}")
    black = black[0] if black is not None and len(black) == 1 else black
    camera_isp._check_levels(black, args.white_level, 12)          # before any frame is read
    shading = None
    if args.lens_shading is not None:
        shading = np.load(args.lens_shading, allow_pickle=False)
        camera_isp._check_shading(shading)                          # (also before any frame is read)
    denoise = None
    if args.raw_denoise is not None:                                # (checked before any frame is read)
        denoise = RawDenoise(args.raw_denoise[0], args.raw_denoise[1], strength=args.denoise_strength,
                             radius=args.denoise_radius)
    highlights = None
    if args.highlights is not None:                                 # (also before any frame is read)
        highlights = Highlights(args.highlights, 0.98 if args.highlights_clip is None else args.highlights_clip)
    elif args.highlights_clip is not None:
        raise ValueError("--highlights-clip needs --highlights {rebuild,clip}")
    dynamic = None
    dyn = dict(threshold=args.dynamic_defects_threshold, slope=args.dynamic_defects_slope,
               tolerate=args.dynamic_defects_tolerate)
    if args.dynamic_defects:                                        # (also before any frame is read)
        dynamic = DynamicDefects(**{k: v for k, v in dyn.items() if v is not None})
    elif any(v is not None for v in dyn.values()):
        raise ValueError("--dynamic-defects-threshold, --dynamic-defects-slope and --dynamic-defects-tolerate need "
                         "--dynamic-defects")
    green = None
    geq = dict(threshold=args.green_equalize_threshold, slope=args.green_equalize_slope,
               strength=args.green_equalize_strength, radius=args.green_equalize_radius, edge=args.green_equalize_edge)
    if args.green_equalize:                                         # (also before any frame is read)
        green = GreenEqualize(**{k: v for k, v in geq.items() if v is not None})
    elif any(v is not None for v in geq.values()):
        raise ValueError("--green-equalize-threshold, -slope, -strength, -radius and -edge need --green-equalize")
    statistics = None
    if args.statistics is not None:                                 # (also before any frame is read)
        parts = args.statistics.lower().split("x")
        if len(parts) != 2 or not all(p.isdigit() for p in parts):
            raise ValueError(f"--statistics takes GHxGW (two integers, e.g. 8x8), got {args.statistics!r}")
        statistics = Statistics(zones=(int(parts[0]), int(parts[1])))
    chromatic = None
    if args.chromatic_aberration is not None:                       # (also before any frame is read)
        k = args.chromatic_aberration
        chromatic = ChromaticAberration(tuple(k[:3]), tuple(k[3:]), center=args.chromatic_center,
                                        norm_radius=args.chromatic_norm_radius)
    elif args.chromatic_center is not None or args.chromatic_norm_radius is not None:
        raise ValueError("--chromatic-center / --chromatic-norm-radius need --chromatic-aberration R0 R1 R2 B0 B1 B2")
    temporal = None
    if args.temporal_denoise is not None:                           # (also before any frame is read)
        temporal = TemporalDenoise(args.temporal_denoise[0], args.temporal_denoise[1],
                                   threshold=3.0 if args.temporal_threshold is None else args.temporal_threshold,
                                   max_weight=0.75 if args.temporal_max_weight is None else args.temporal_max_weight)
    elif args.temporal_threshold is not None or args.temporal_max_weight is not None:
        raise ValueError("--temporal-threshold / --temporal-max-weight need --temporal-denoise GAIN READ_NOISE")
    local_tonemap = None
    if args.local_tonemap is not None:                              # (also before any frame is read)
        local_tonemap = LocalTonemap(args.local_tonemap,
                                     floor=2.0 ** -10 if args.local_tonemap_floor is None else args.local_tonemap_floor,
                                     cell=32 if args.local_tonemap_cell is None else args.local_tonemap_cell)
    elif args.local_tonemap_floor is not None or args.local_tonemap_cell is not None:
        raise ValueError("--local-tonemap-floor / --local-tonemap-cell need --local-tonemap STRENGTH")
    sharpen = None
    if args.sharpen is not None:                                    # (also before any frame is read)
        sharpen = Sharpen(args.sharpen, radius=args.sharpen_radius, threshold=args.sharpen_threshold,
                          overshoot=args.sharpen_overshoot)
    elif (args.sharpen_radius, args.sharpen_threshold, args.sharpen_overshoot) != (1, 0, None):
        raise ValueError("--sharpen-radius / --sharpen-threshold / --sharpen-overshoot need --sharpen AMOUNT")
    local_contrast = None
    if args.local_contrast is not None:                             # (also before any frame is read)
        clip = 2.0 if args.local_contrast_clip is None else (args.local_contrast_clip or None)
        local_contrast = LocalContrast(tuple(args.local_contrast_tiles or (8, 8)), clip, args.local_contrast)
    elif args.local_contrast_tiles is not None or args.local_contrast_clip is not None:
        raise ValueError("--local-contrast-tiles / --local-contrast-clip need --local-contrast STRENGTH")
    chroma_denoise = None
    if args.chroma_denoise is not None:                             # (also before any frame is read)
        tl, tc = args.chroma_denoise_thresholds or (8, 12)
        chroma_denoise = ChromaDenoise(2 if args.chroma_denoise_radius is None else args.chroma_denoise_radius, tl, tc,
                                       args.chroma_denoise)
    elif args.chroma_denoise_radius is not None or args.chroma_denoise_thresholds is not None:
        raise ValueError("--chroma-denoise-radius / --chroma-denoise-thresholds need --chroma-denoise STRENGTH")
    luma_denoise = None
    if args.luma_denoise is not None:                               # (also before any frame is read)
        t0, t1 = args.luma_denoise_thresholds or (6, 6)
        luma_denoise = LumaDenoise(2 if args.luma_denoise_radius is None else args.luma_denoise_radius, t0, t1,
                                   args.luma_denoise)
    elif args.luma_denoise_radius is not None or args.luma_denoise_thresholds is not None:
        raise ValueError("--luma-denoise-radius / --luma-denoise-thresholds need --luma-denoise STRENGTH")
    color_lut = None
    if args.color_lut is not None:                                  # (read and checked before any frame is read)
        color_lut = ColorLut.from_cube(args.color_lut, 1.0 if args.color_lut_strength is None else args.color_lut_strength)
    elif args.color_lut_strength is not None:
        raise ValueError("--color-lut-strength needs --color-lut FILE.cube")
    index = ScanIndex.of_scan(args.scan) if args.scan is not None else ScanIndex.of_directory(args.images)
    coords = {} if args.defect_pixels is None else load_defect_pixels(args.defect_pixels, index.cameras, args.width)
    calib = {} if args.lens_distortion is None else load_lens_distortion(args.lens_distortion, index.cameras)
    maps = None                                                     # one DefectMap per camera, once the height is known
    lenses = None                                                   # (and one LensDistortion)
    print(f"{len(index.cameras)} camera(s) {[c.name for c in index.cameras]}, {len(index.frames)} frame(s) each")
    device = torch.device(args.device)
    isp = camera_isp.Camera32(bayer.BayerPattern.RGGB, transform=args.transform, moving_alpha=args.moving_alpha,
                              resize_width=args.resize_width, correct_colors=args.correct_colors, device=device,
                              black_level=black, white_level=args.white_level, lens_shading=shading,
                              auto_white_balance=args.auto_white_balance, raw_denoise=denoise, sharpen=sharpen,
                              local_contrast=local_contrast, chroma_denoise=chroma_denoise, color_lut=color_lut,
                              highlights=highlights, chromatic_aberration=chromatic, temporal_denoise=temporal,
                              local_tonemap=local_tonemap, luma_denoise=luma_denoise,
                              demosaic=None if args.demosaic is None else Demosaic(args.demosaic),
                              resample=None if args.resample is None else Resample(args.resample),
                              dynamic_defects=dynamic, green_equalize=green, statistics=statistics)
    # temporal noise reduction: the state of each camera folder, for the whole scan
    histories = [TemporalHistory() if temporal is not None else None for _ in index.cameras]
    row_bytes = args.width * 3 // 2
    if args.write is not None:
        args.write.mkdir(exist_ok=True, parents=True)
    done = 0
    for name, raws in index.groups(partial(ingest.load_raw_bytes, device=device), args.reverse):
        for raw in raws:
            assert raw.numel() % row_bytes == 0, f"{name}: {raw.numel()} bytes is not a whole number of {row_bytes}-byte rows"
        frames = [raw.view(-1, row_bytes) for raw in raws]
        if maps is None:
            shape = (frames[0].shape[0], args.width)
            maps = [DefectMap(coords[c.name], shape) if c.name in coords else None for c in index.cameras]
            lenses = [LensDistortion(shape=shape, **calib[c.name]) if c.name in calib else None for c in index.cameras]
        images, measured = [], []
        for f, m, ln, hist in zip(frames, maps, lenses, histories):
            images.append(isp.load_packed12(f, ids_format=args.ids_format, defects=m, undistort=ln, history=hist))
            measured.extend(isp.frame_statistics or [])
        outputs = isp.tonemap_reinhard(images, gamma=args.gamma, intensity=args.intensity,
                                       color_adapt=args.color_adapt, light_adapt=args.light_adapt)
        if args.write is not None:
            target = args.write / (Path(name).stem + ".png")
            write_png(target, tile_grid(outputs, args.rows).cpu().numpy())
            print(f"wrote {target}")
            if statistics is not None:
                target = args.write / (Path(name).stem + ".stats.json")
                target.write_text(json.dumps(statistics_report(statistics, [c.name for c in index.cameras], measured)))
                print(f"wrote {target}")
        done += 1
    print(f"processed {done} frame group(s) from {len(index.cameras)} camera(s)")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
