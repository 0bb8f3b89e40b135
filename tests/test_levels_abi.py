"""Sensor levels without a GPU: the C entry points and the Python call surface reject bad levels before any launch."""
import ctypes

import pytest

from taichi_image_amd import camera_isp


def test_levels_entry_points_validate_on_the_host():
    from taichi_image_amd import _native
    L = _native.lib()
    assert L.mi_isp_version() >= 1100
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    one = (ctypes.c_void_p * 1)(p)
    for black, white, bits in (([0, 0, 0, 4095], 4095, 12), ([-1, 0, 0, 0], 4095, 12), ([0] * 4, 4096, 12),
                               ([0] * 4, 70000, 16), ([10, 10, 10, 10], 10, 16)):
        lv = _native.levels_arg(black, white)
        assert L.mi_isp_load_packed_levels(p, p, 4, 8, bits, 0, 0, None, 2, 4, 8, 0.0, lv, None) != 0
        assert b"level" in L.mi_isp_last_error()
        assert L.mi_isp_load_packed_metered_levels(p, p, 4, 8, bits, 0, 0, None, 2, 4, 8, 0.0, p, 8, lv, None) != 0
        assert L.mi_isp_load_packed_batch_levels(one, one, None, 1, 4, 8, bits, 0, 0, None, 2, 4, 8, 0.0, 8, lv, None) != 0
        assert b"level" in L.mi_isp_last_error()
    lv = _native.levels_arg([0, 0, 0, 65535], 65535)
    assert L.mi_isp_load_convert_levels(p, p, 4, 8, 0, 2, lv, None) != 0
    assert b"level" in L.mi_isp_last_error()
    assert L.mi_isp_load_convert_levels(p, p, 4, 8, 1, 2, _native.levels_arg([0] * 4, 100), None) != 0   # f32 source
    assert b"u16" in L.mi_isp_last_error()


def test_check_levels():
    assert camera_isp._check_levels(None, None) is None
    assert camera_isp._check_levels(64, None, 12) == ([64] * 4, 4095)
    assert camera_isp._check_levels([1, 2, 3, 4], 1000, 12) == ([1, 2, 3, 4], 1000)
    assert camera_isp._check_levels(None, 60000, 16) == ([0] * 4, 60000)
    for black, white, bits in ((4095, None, 12), (-1, None, 16), ([1, 2], None, 16), (1.5, None, 16), (True, None, 16),
                               (0, 5000, 12), (0, 0, 16), (10, 10, 16)):
        with pytest.raises(ValueError):
            camera_isp._check_levels(black, white, bits)
