"""taichi_image_amd -- MI355X-native camera-ISP hot path behind taichi_image's call surface.

    from taichi_image_amd import camera_isp, bayer, packed, tonemap, interpolate

mirror the modules of uc-vision/taichi_image; every op dispatches through ctypes into
libmi355_isp.so (hand-written HIP for gfx950).  There is no CPU fallback.
"""
from . import types  # noqa: F401
from . import packed, bayer, interpolate, tonemap, camera_isp, pipeline, distributed, color, ingest, defects, lens, white_balance, denoise, sharpen, local_contrast, chroma_denoise, luma_denoise, color_lut, highlights, chromatic, temporal, exposure_merge, local_tonemap, demosaic, resample, dynamic_defects, green_equalize, statistics  # noqa: F401
from .bayer import BayerPattern  # noqa: F401
from .demosaic import Demosaic  # noqa: F401
from .resample import Resample, check_resample  # noqa: F401
from .interpolate import ImageTransform  # noqa: F401
from .camera_isp import Camera16, Camera32  # noqa: F401
from .defects import DefectMap, find_defects  # noqa: F401
from .lens import LensDistortion  # noqa: F401
from .white_balance import AutoWhiteBalance  # noqa: F401
from .denoise import RawDenoise  # noqa: F401
from .sharpen import Sharpen  # noqa: F401
from .local_contrast import LocalContrast  # noqa: F401
from .chroma_denoise import ChromaDenoise  # noqa: F401
from .luma_denoise import LumaDenoise  # noqa: F401
from .color_lut import ColorLut  # noqa: F401
from .highlights import Highlights  # noqa: F401
from .dynamic_defects import DynamicDefects, check_dynamic_defects, find_defects_dynamic  # noqa: F401
from .green_equalize import GreenEqualize, check_green_equalize, equalize_cfa  # noqa: F401
from .statistics import Statistics, FrameStatistics, check_statistics, statistics_cfa  # noqa: F401
from .chromatic import ChromaticAberration  # noqa: F401
from .temporal import TemporalDenoise, TemporalHistory, check_temporal_denoise, temporal_cfa  # noqa: F401
from .exposure_merge import ExposureMerge, check_exposure_merge, merge_cfa  # noqa: F401
from .local_tonemap import LocalTonemap, check_local_tonemap  # noqa: F401

__version__ = "0.1.0"
