"""The overlay entry points (include/vf_hip.h) are declared, listed in cabi.SYMBOLS, exported by libvf_hip.so, and argument errors
that need no device are reported as such (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_add_points": ["t", "xyz", "n", "size_px", "rgba", "default_size", "default_rgba", "shape", "drape", "layer_id"],
                "vf_terrain_add_lines": ["t", "xyz", "path_offsets", "npaths", "width_px", "rgba", "cap", "drape", "layer_id"],
                "vf_terrain_clear_overlays": ["t"]}


def test_overlay_entry_points_are_declared_listed_and_exported():
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("SHAPE", (("CIRCLE", 0), ("SQUARE", 1)))
    abi.check_defines("CAP", (("BUTT", 0), ("SQUARE", 1), ("ROUND", 2)))


def test_overlay_calls_refuse_a_null_handle():
    one, two = np.zeros(3, np.float32), np.zeros(6, np.float32)
    offs = np.array([0, 2], np.uint32)
    col = ctypes.cast((ctypes.c_uint8 * 4)(255, 255, 255, 255), ctypes.c_void_p)
    abi.check_null_refusals([("vf_terrain_add_points", (one.ctypes.data, 1, None, None, 4.0, col, 0, 0, None)),
                             ("vf_terrain_clear_overlays", ()),
                             ("vf_terrain_add_lines", (two.ctypes.data, offs.ctypes.data, 1, 2.0, col, 2, 0, None))])


def test_pack_lines_and_argument_rules():
    pytest.importorskip("vulkan_forge_amd._vulkan_forge")
    import vulkan_forge as vf
    from vulkan_forge_amd import _overlays as ov
    coords, offs = vf.pack_lines([np.array([[0, 0, 0], [0, 0, 0], [1, 2, 3], [1, 2, 3], [4, 5, 6]], np.float64),
                                  np.array([[1, 1, 1], [2, 2, 2]], np.float32)])
    assert coords.dtype == np.float32 and coords.shape == (5, 3)
    assert offs.dtype == np.uint32 and offs.tolist() == [0, 3, 5]
    assert coords[:3].tolist() == [[0, 0, 0], [1, 2, 3], [4, 5, 6]]
    with pytest.raises(ValueError, match="fewer than 2"):
        vf.pack_lines([np.array([[1, 1, 1], [1, 1, 1]], np.float32)])
    with pytest.raises(ValueError, match="non-finite"):
        vf.pack_lines([np.array([[1, 1, 1], [np.nan, 1, 1]], np.float32)])
    with pytest.raises(TypeError, match="float32 or float64"):
        vf.pack_lines([np.array([[1, 1, 1], [2, 1, 1]], np.int32)])
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        vf.pack_lines([np.zeros((4, 2), np.float32)])
    pts = np.zeros((3, 3), np.float32)
    with pytest.raises(TypeError, match="float32 or float64"):
        ov.point_args(pts.astype(np.int64), 4.0, (1, 2, 3, 4), "circle")
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        ov.point_args(np.zeros((3, 4), np.float32), 4.0, (1, 2, 3, 4), "circle")
    with pytest.raises(ValueError, match="shape must be"):
        ov.point_args(pts, 4.0, (1, 2, 3, 4), "star")
    with pytest.raises(ValueError, match="cap must be"):
        ov.line_args([np.eye(3)], 2.0, (1, 2, 3, 4), "arrow")
    with pytest.raises(TypeError, match="uint8"):
        ov.point_args(pts, 4.0, np.zeros((3, 4), np.int32), "circle")
    with pytest.raises(ValueError, match=r"\(3, 4\)"):
        ov.point_args(pts, 4.0, np.zeros((2, 4), np.uint8), "circle")
    with pytest.raises(ValueError, match="0..255"):
        ov.point_args(pts, 4.0, (1, 2, 3, 256), "circle")
    with pytest.raises(ValueError, match=r"\(3,\)"):
        ov.point_args(pts, np.ones(2, np.float32), (1, 2, 3, 4), "circle")
    p, dsize, sizes, dcol, cols, shape = ov.point_args(pts.astype(np.float64), np.full(3, 2.0), np.zeros((3, 4), np.uint8), "square")
    assert p.dtype == np.float32 and sizes.dtype == np.float32 and cols.shape == (3, 4) and shape == 1
