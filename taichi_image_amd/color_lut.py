"""3D colour LUT (an extension): tetrahedral interpolation in an N x N x N table on the u8 images the tonemaps return, defined
in integer arithmetic so that its output is the contract's bit for bit ("Colour LUT").

`Camera16/32(color_lut=ColorLut(...))` maps every u8 RGB output of the tonemaps and of process_packed12 through the table,
first of the output operators (tone curve -> colour LUT -> chroma noise reduction -> local contrast -> sharpening);
`apply_lut` maps an (H, W, 3) u8 image on its own.  `ColorLut.from_cube` reads the Adobe / Resolve .cube text form.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import _native, _u8_stage as _u8, types

MIN_POINTS, MAX_POINTS = 2, 65


def _quantise(x):
    """u8 codes of float values in [0, 1], in float64: floor(clip(x, 0, 1) * 255 + 0.5)."""
    x = np.asarray(x, np.float64)
    if not np.isfinite(x).all():
        raise ValueError("ColorLut.table must be finite")
    return np.floor(np.clip(x, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


class ColorLut:
    """A 3D colour lookup table.  table is (N, N, N, 3), 2 <= N <= 65, indexed [r][g][b]: the output colour (R, G, B) at input
    (r, g, b) * 255 / (N - 1); u8, or float in [0, 1] quantised once on the host (floor(clip(x, 0, 1) * 255 + 0.5) in
    float64).  The array is copied and read-only.  strength (0 .. 1) blends between the input and the table's colour,
    quantised once to 1/64."""

    def __init__(self, table, strength=1.0):
        if isinstance(table, torch.Tensor):
            table = table.detach().cpu().numpy()
        if not isinstance(table, np.ndarray):
            raise ValueError(f"ColorLut.table must be an array, got {type(table).__name__}")
        if (table.ndim != 4 or table.shape[3] != 3 or not table.shape[0] == table.shape[1] == table.shape[2]
                or not MIN_POINTS <= table.shape[0] <= MAX_POINTS):
            raise ValueError(f"ColorLut.table must be (N, N, N, 3) with N in {MIN_POINTS} .. {MAX_POINTS}, got shape "
                             f"{tuple(table.shape)}")
        if table.dtype == np.uint8:
            t = table.copy()
        elif np.issubdtype(table.dtype, np.floating):
            t = _quantise(table)
        else:
            raise ValueError(f"ColorLut.table must be u8 or float, got {table.dtype}")
        t = np.ascontiguousarray(t)
        t.setflags(write=False)
        _u8.number("ColorLut", "strength", strength, 0, 1)
        self._table = t
        self._strength = float(strength)
        self._device_tables = {}

    @property
    def table(self) -> np.ndarray:
        """The (N, N, N, 3) u8 table, read-only."""
        return self._table

    @property
    def n_points(self) -> int:
        """N, the points per axis."""
        return self._table.shape[0]

    @property
    def strength(self) -> float:
        return self._strength

    @property
    def strength_q6(self) -> int:
        """S = floor(strength * 64 + 0.5): the weight the operator multiplies with, 0 .. 64."""
        return _u8.q6(self._strength)

    def __eq__(self, other):
        return (isinstance(other, ColorLut) and self._strength == other._strength
                and np.array_equal(self._table, other._table))

    __hash__ = None

    def __repr__(self):
        return f"ColorLut(n_points={self.n_points}, strength={self._strength})"

    def packed(self) -> np.ndarray:
        """The device form: N^3 dwords, entry (r * N + g) * N + b = R | G << 8 | B << 16."""
        t = self._table.astype(np.uint32)
        return (t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16)).reshape(-1)

    def _device_table(self, device: torch.device) -> torch.Tensor:
        """The packed table on `device`: made once per table and device, its upload ordered on the device's current stream
        (launches on other streams are the caller's to order behind it, as with any tensor)."""
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        t = self._device_tables.get(key)
        if t is None:
            t = torch.from_numpy(self.packed().view(np.int32)).to(device)
            self._device_tables[key] = t
        return t

    def _arg(self) -> "_native.ColorLut":
        """The mi_isp_color_lut of these settings."""
        return _native.ColorLut(self.n_points, self.strength_q6)

    @staticmethod
    def identity(n_points: int, strength=1.0) -> "ColorLut":
        """The table that returns every colour unchanged: T[r][g][b] = (q(r), q(g), q(b)), q(k) = (2 * 255 k + (N - 1)) //
        (2 (N - 1)), the code nearest to 255 k / (N - 1)."""
        if isinstance(n_points, bool) or not isinstance(n_points, (int, np.integer)) or not MIN_POINTS <= n_points <= MAX_POINTS:
            raise ValueError(f"ColorLut.identity: n_points must be an integer in {MIN_POINTS} .. {MAX_POINTS}, got {n_points!r}")
        n = int(n_points)
        q = ((2 * 255 * np.arange(n) + (n - 1)) // (2 * (n - 1))).astype(np.uint8)
        t = np.empty((n, n, n, 3), np.uint8)
        t[..., 0] = q[:, None, None]
        t[..., 1] = q[None, :, None]
        t[..., 2] = q[None, None, :]
        return ColorLut(t, strength)

    @staticmethod
    def from_cube(path_or_text, strength=1.0) -> "ColorLut":
        """The table of a .cube file (Adobe / Resolve text form), given as a path or as the text itself (a string with a
        line break).  Accepted: `#` comments, blank lines, TITLE, LUT_3D_SIZE N, DOMAIN_MIN 0 0 0, DOMAIN_MAX 1 1 1,
        LUT_3D_INPUT_RANGE 0 1, then N^3 rows of three floats with R varying fastest.  ValueError for any other domain,
        LUT_1D_SIZE, any other keyword, a wrong number of rows, a malformed row and N outside 2 .. 65."""
        if isinstance(path_or_text, (str, os.PathLike)) and not (isinstance(path_or_text, str) and "\n" in path_or_text):
            with open(path_or_text, "r", encoding="utf-8", errors="replace") as f:
                text = f.read()
        elif isinstance(path_or_text, str):
            text = path_or_text
        else:
            raise ValueError(f"from_cube takes a path or the text of a .cube file, got {type(path_or_text).__name__}")
        n = None
        rows = []

        def floats(fields, count, line):
            if len(fields) != count:
                raise ValueError(f".cube: malformed line {line!r}")
            try:
                vals = [float(f) for f in fields]
            except ValueError:
                raise ValueError(f".cube: malformed line {line!r}") from None
            if not all(math.isfinite(v) for v in vals):
                raise ValueError(f".cube: non-finite value in line {line!r}")
            return vals

        for raw in text.splitlines():
            line = raw.strip()
            if not line or line.startswith("#"):
                continue
            head = line.split()[0]
            if head == "TITLE":
                continue
            if head == "LUT_1D_SIZE":
                raise ValueError(".cube: LUT_1D_SIZE: a 1D table is not a 3D colour LUT")
            if head == "LUT_3D_SIZE":
                fields = line.split()
                if len(fields) != 2 or not fields[1].isdigit() or n is not None or rows:
                    raise ValueError(f".cube: malformed line {line!r}")
                n = int(fields[1])
                if not MIN_POINTS <= n <= MAX_POINTS:
                    raise ValueError(f".cube: LUT_3D_SIZE {n} outside {MIN_POINTS} .. {MAX_POINTS}")
                continue
            if head in ("DOMAIN_MIN", "DOMAIN_MAX", "LUT_3D_INPUT_RANGE"):
                want = {"DOMAIN_MIN": [0.0] * 3, "DOMAIN_MAX": [1.0] * 3, "LUT_3D_INPUT_RANGE": [0.0, 1.0]}[head]
                if rows or floats(line.split()[1:], len(want), line) != want:
                    raise ValueError(f".cube: only the domain 0 .. 1 is supported, got {line!r}")
                continue
            if head[0].isalpha() and head.lower() not in ("nan", "inf", "infinity"):
                raise ValueError(f".cube: unknown keyword in line {line!r}")
            if n is None:
                raise ValueError(f".cube: data before LUT_3D_SIZE: {line!r}")
            rows.append(floats(line.split(), 3, line))
        if n is None:
            raise ValueError(".cube: no LUT_3D_SIZE")
        if len(rows) != n ** 3:
            raise ValueError(f".cube: {len(rows)} rows for LUT_3D_SIZE {n} ({n ** 3} expected)")
        # R varies fastest: the rows are [b][g][r]
        table = np.asarray(rows, np.float64).reshape(n, n, n, 3).transpose(2, 1, 0, 3)
        return ColorLut(table, strength)


def check_color_lut(value):
    """The ColorLut of a constructor / set() argument, None for None; ValueError otherwise."""
    return _u8.check_setting(value, ColorLut, "color_lut")


def apply(images, lut: ColorLut, inplace=False):
    """The operator on the u8 device tensors `images` ((H, W, 3), one shape, contiguous, one device).  inplace=True
    overwrites and returns `images` (the operator is pointwise), else new tensors come back.  One launch per 32 images on
    the device's current stream, no host synchronisation."""
    H, W = images[0].shape[:2]
    table = lut._device_table(images[0].device).data_ptr() if H * W else None
    return _u8.apply_batch(images, "mi_isp_color_lut_rgb_batch", None, table, inplace=inplace, extra=(lut._arg(),))


def apply_lut(image, lut: ColorLut):
    """The operator on an (H, W, 3) u8 RGB image.  numpy in gives numpy out, torch in gives torch out on the same device
    (always a new array).  DESIGN.md 3, "Colour LUT"."""
    if not isinstance(lut, ColorLut):
        raise ValueError(f"lut must be a ColorLut, got {type(lut).__name__}")
    if not isinstance(image, (np.ndarray, torch.Tensor)):
        raise ValueError(f"apply_lut takes an array, got {type(image).__name__}")
    if image.dtype not in (np.uint8, torch.uint8):
        raise ValueError(f"apply_lut takes a u8 image, got {image.dtype}")
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError(f"apply_lut takes an (H, W, 3) image, got shape {tuple(image.shape)}")
    dev = types.to_device(image)
    return types.from_device(apply([dev], lut)[0], image)
