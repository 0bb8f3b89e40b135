"""Lens distortion correction: per-camera calibrations for the ISP's raw loaders and for interpolate.undistort (an
extension; DESIGN.md 3, "Lens distortion").

A LensDistortion maps each pixel of an undistorted output to the source coordinates (us, vs) of the distorted H x W
image it is sampled from.  The analytic form is OpenCV's pinhole model: camera matrix K = [[fx, 0, cx], [0, fy, cy],
[0, 0, 1]], distortion coefficients in OpenCV order - (k1, k2, p1, p2), (k1, k2, p1, p2, k3) or the rational
(k1, k2, p1, p2, k3, k4, k5, k6) - and the output camera matrix new_K (K by default).  The kernel evaluates it per pixel
in f32; it builds no table.  The table form (from_map) takes an (Hd, Wd, 2) f32 array of source coordinates in OpenCV's
map_x / map_y order, e.g. from cv2.initUndistortRectifyMap or a fisheye model: it is uploaded once per device and cached
on the object, so a repeat call makes no host-to-device copy and can be captured in a graph.

distortion_map gives the (us, vs) the kernel computes, on the host, in NumPy f32 with the same operations.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native

f32 = np.float32
BORDERS = {"constant": 0, "replicate": 1}


def _camera_matrix(K, what):
    """(fx, fy, cx, cy) of a 3 x 3 camera matrix [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]; ValueError otherwise."""
    k = np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K)
    if k.shape != (3, 3) or k.dtype == np.bool_ or not np.issubdtype(k.dtype, np.number) or np.iscomplexobj(k):
        raise ValueError(f"{what} must be a real 3 x 3 matrix, got {k.dtype} {k.shape}")
    k = k.astype(np.float64)
    with np.errstate(over="ignore"):
        finite = np.all(np.isfinite(k)) and np.all(np.isfinite(k.astype(f32)))
    if not finite:
        raise ValueError(f"{what} must be finite (in f32 too)")
    if k[0, 1] != 0 or k[1, 0] != 0 or k[2, 0] != 0 or k[2, 1] != 0 or k[2, 2] != 1:
        raise ValueError(f"{what} must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew), got {k.tolist()}")
    fx, fy, cx, cy = float(k[0, 0]), float(k[1, 1]), float(k[0, 2]), float(k[1, 2])
    with np.errstate(over="ignore"):
        ok = fx > 0 and fy > 0 and f32(fx) > 0 and f32(fy) > 0 and np.isfinite(f32(1.0 / fx)) and np.isfinite(f32(1.0 / fy))
    if not ok:
        raise ValueError(f"{what}: focal lengths must be positive, got fx {fx}, fy {fy}")
    return fx, fy, cx, cy


def _coefficients(dist):
    d = np.asarray(dist.detach().cpu().numpy() if isinstance(dist, torch.Tensor) else dist)
    if d.dtype == np.bool_ or not np.issubdtype(d.dtype, np.number) or np.iscomplexobj(d):
        raise ValueError(f"dist must hold real numbers, got {d.dtype}")
    d = d.astype(np.float64).reshape(-1) if d.ndim == 2 and 1 in d.shape else d.astype(np.float64)
    if d.ndim != 1 or len(d) not in (4, 5, 8):
        raise ValueError(f"dist must hold 4, 5 or 8 coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got shape {d.shape}")
    with np.errstate(over="ignore"):
        finite = np.all(np.isfinite(d)) and np.all(np.isfinite(d.astype(f32)))
    if not finite:
        raise ValueError("dist coefficients must be finite (in f32 too)")
    return tuple(float(v) for v in d)


def _shape(shape):
    if not (isinstance(shape, (tuple, list)) and len(shape) == 2):
        raise ValueError(f"shape must be (H, W), got {shape!r}")
    for v in shape:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"shape must hold integers, got {shape!r}")
    H, W = int(shape[0]), int(shape[1])
    if not (0 < H < 2 ** 24 and 0 < W < 2 ** 24):
        raise ValueError(f"shape {(H, W)} must be positive (and under 2**24)")
    return H, W


def _border(border):
    if border not in BORDERS:
        raise ValueError(f"border must be one of {sorted(BORDERS)}, got {border!r}")
    return border


def _scale2(scale):
    if np.isscalar(scale):
        s = (float(scale), float(scale))
    else:
        s = tuple(float(v) for v in scale)
        if len(s) != 2:
            raise ValueError("scale must be a scalar or a (row, col) pair")
    if not all(np.isfinite(v) and f32(v) > 0 for v in s):
        raise ValueError(f"scale must be positive and finite, got {scale!r}")
    return s


class LensDistortion:
    """The lens of one camera, for its (H, W) frames.

    LensDistortion(K, dist, shape, new_K=None, border="constant"): the analytic form (OpenCV's model; see the module).
    LensDistortion.from_map(map_xy, shape, border="constant"): the table form.
    border: "constant" (0 outside the source frame) or "replicate" (the edge pixels).  ValueError for anything else, for
    a K or new_K that is not [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with finite values and fx, fy > 0, for a dist of
    another length than 4, 5 or 8, and for non-finite coefficients."""

    def __init__(self, K, dist, shape, new_K=None, border="constant"):
        self._shape = _shape(shape)
        self._K = _camera_matrix(K, "K")
        self._new_K = self._K if new_K is None else _camera_matrix(new_K, "new_K")
        self._dist = _coefficients(dist)
        self._border = _border(border)
        self._table = None
        self._dev = {}                                   # device index -> the table on that device

    @classmethod
    def from_map(cls, map_xy, shape, border="constant") -> "LensDistortion":
        """The table form: map_xy is an (Hd, Wd, 2) f32 array (numpy or torch) of source coordinates (us, vs) of a
        shape = (H, W) source; copied on the host once."""
        m = map_xy.detach().cpu().numpy() if isinstance(map_xy, torch.Tensor) else np.asarray(map_xy)
        if m.dtype != np.float32:
            raise ValueError(f"map_xy must be float32, got {m.dtype}")
        if m.ndim != 3 or m.shape[2] != 2 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError(f"map_xy must be (Hd, Wd, 2) (us, vs), got shape {m.shape}")
        self = cls.__new__(cls)
        self._shape = _shape(shape)
        self._K = self._new_K = self._dist = None
        self._border = _border(border)
        self._table = np.ascontiguousarray(m).copy()
        self._table.setflags(write=False)
        self._dev = {}
        return self

    @property
    def shape(self):
        """(H, W) of the distorted source frames."""
        return self._shape

    @property
    def border(self) -> str:
        return self._border

    @property
    def is_table(self) -> bool:
        return self._table is not None

    @property
    def table(self):
        """The (Hd, Wd, 2) f32 table of the table form (read-only), None for the analytic form."""
        return self._table

    @property
    def table_shape(self):
        """(Hd, Wd) of the table form's output, None for the analytic form."""
        return None if self._table is None else self._table.shape[:2]

    @property
    def K(self):
        return None if self._K is None else _matrix(self._K)

    @property
    def new_K(self):
        return None if self._new_K is None else _matrix(self._new_K)

    @property
    def dist(self):
        return self._dist

    def __repr__(self) -> str:
        if self.is_table:
            return f"LensDistortion.from_map({self._table.shape}, shape={self._shape}, border={self._border!r})"
        return f"LensDistortion(K={self._K}, dist={self._dist}, shape={self._shape}, border={self._border!r})"

    def distortion_map(self, Hd: int, Wd: int, scale=1.0) -> np.ndarray:
        """The source coordinates (us, vs) of every pixel of an Hd x Wd output at output scale `scale` (a scalar or
        (row, col); no half-pixel offset) as the kernel computes them: an (Hd, Wd, 2) f32 array.  The table form
        returns a copy of its table (ValueError for another output shape)."""
        Hd, Wd = int(Hd), int(Wd)
        if self.is_table:
            if (Hd, Wd) != tuple(self.table_shape):
                raise ValueError(f"the lens table is {self.table_shape[0]} x {self.table_shape[1]}, not {Hd} x {Wd}")
            return self._table.copy()
        s0, s1 = (f32(v) for v in _scale2(scale))
        fx, fy, cx, cy = (f32(v) for v in self._K)
        nfx, nfy, ncx, ncy = self._new_K
        ifx, ify = f32(1.0 / nfx), f32(1.0 / nfy)
        ncx, ncy = f32(ncx), f32(ncy)
        d = [f32(v) for v in self._dist] + [f32(0)] * (8 - len(self._dist))
        k1, k2, p1, p2, k3, k4, k5, k6 = d
        one, two = f32(1), f32(2)
        u = np.arange(Wd, dtype=np.int32).astype(f32) / s1
        v = np.arange(Hd, dtype=np.int32).astype(f32) / s0
        x = ((u - ncx) * ifx)[None, :]
        y = ((v - ncy) * ify)[:, None]
        r2 = x * x + y * y
        radial = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        if len(self._dist) == 8:
            radial = radial / (one + r2 * (k4 + r2 * (k5 + r2 * k6)))
        xd = x * radial + (two * p1) * x * y + p2 * (r2 + two * x * x)
        yd = y * radial + p1 * (r2 + two * y * y) + (two * p2) * x * y
        out = np.empty((Hd, Wd, 2), f32)
        out[..., 0] = fx * xd + cx
        out[..., 1] = fy * yd + cy
        return out

    # ---- the library's arguments ------------------------------------------------------------------------------------
    def _arg(self) -> "_native.Lens":
        fx, fy, cx, cy = self._K
        nfx, nfy, ncx, ncy = self._new_K
        d = list(self._dist) + [0.0] * (8 - len(self._dist))
        return _native.Lens(fx, fy, cx, cy, nfx, nfy, ncx, ncy, (_native.c_double * 8)(*d), len(self._dist),
                            BORDERS[self._border])

    def _table_dev(self, device: torch.device) -> torch.Tensor:
        """The table on `device`, uploaded by the first call and cached."""
        key = device.index if device.index is not None else torch.cuda.current_device()
        t = self._dev.get(key)
        if t is None:
            with torch.cuda.device(key):
                t = torch.from_numpy(self._table.copy()).to(torch.device("cuda", key))
            self._dev[key] = t
        return t


def _matrix(k):
    fx, fy, cx, cy = k
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def check_lens(lens, shape, out_shape=None):
    """None for no correction, else the lens; ValueError for a lens of another frame shape, or a table whose output shape
    is not out_shape = (Hd, Wd)."""
    if lens is None:
        return None
    if not isinstance(lens, LensDistortion):
        raise ValueError(f"undistort must be a LensDistortion or None, got {type(lens).__name__}")
    if tuple(lens.shape) != tuple(shape):
        raise ValueError(f"lens of a {lens.shape[0]} x {lens.shape[1]} frame given for a {shape[0]} x {shape[1]} frame")
    if lens.is_table and out_shape is not None and tuple(lens.table_shape) != tuple(out_shape):
        raise ValueError(f"lens table of a {lens.table_shape[0]} x {lens.table_shape[1]} output given for a "
                         f"{out_shape[0]} x {out_shape[1]} output")
    return lens


def apply(lenses, srcs, dsts, H, W, Hd, Wd, s0, s1, in_code, out_code, device):
    """dsts[i] = the remap of srcs[i] ((H, W, 3) device tensors) through lenses[i] (none None; checked with check_lens):
    the analytic lenses in one mi_isp_undistort_batch call, each table through mi_isp_remap, on the device's stream."""
    L = _native.lib()
    stream = _native.stream_ptr(device)
    ana = [i for i, m in enumerate(lenses) if not m.is_table]
    for i, m in enumerate(lenses):
        if m.is_table:
            _native.check(L.mi_isp_remap(srcs[i].data_ptr(), dsts[i].data_ptr(), m._table_dev(device).data_ptr(), H, W, Hd,
                                         Wd, in_code, out_code, BORDERS[m.border], stream))
    if not ana:
        return
    if len(ana) == 1:
        i = ana[0]
        _native.check(L.mi_isp_undistort(srcs[i].data_ptr(), dsts[i].data_ptr(), H, W, Hd, Wd, float(s0), float(s1),
                                         in_code, out_code, lenses[i]._arg(), stream))
        return
    args = [lenses[i]._arg() for i in ana]                                       # (kept alive through the call)
    p_lens = (_native.c_void_p * len(args))(*[_native.ctypes.addressof(a) for a in args])
    _native.check(L.mi_isp_undistort_batch(_native.ptr_array([srcs[i] for i in ana]), _native.ptr_array([dsts[i] for i in ana]),
                                           len(ana), H, W, Hd, Wd, float(s0), float(s1), in_code, out_code, p_lens, stream))
