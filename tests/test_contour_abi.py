"""The contour entry points (include/vf_hip.h) are declared, listed in cabi.SYMBOLS, exported by libvf_hip.so, refuse a NULL handle,
and add_contours' argument rules (vulkan_forge_amd/_overlays.py contour_args) hold (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_add_contours": ["t", "levels", "nlevels", "width_px", "rgba", "lift", "join", "occlude", "depth_bias", "layer_id", "nsegments"],
                "vf_terrain_height_bounds": ["t", "lo", "hi"],
                "vf_terrain_layer_primitive_count": ["t", "layer_id", "count"]}


def test_contour_entry_points_are_declared_listed_and_exported():
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("JOIN", (("ROUND", 0), ("NONE", 1)))


def test_contour_calls_refuse_a_null_handle():
    lv = np.float32([0.0, 1.0])
    col = ctypes.cast((ctypes.c_uint8 * 4)(0, 0, 0, 255), ctypes.c_void_p)
    lo, hi, n = ctypes.c_float(), ctypes.c_float(), ctypes.c_uint32()
    abi.check_null_refusals([("vf_terrain_add_contours", (lv.ctypes.data, 2, 1.0, col, 0.0, 0, 0, 0.01, None, None)),
                             ("vf_terrain_height_bounds", (ctypes.byref(lo), ctypes.byref(hi))),
                             ("vf_terrain_layer_primitive_count", (0, ctypes.byref(n)))])


def test_scene_and_terrain_spike_have_the_methods():
    pytest.importorskip("vulkan_forge_amd._vulkan_forge")
    import vulkan_forge as vf
    for cls in (vf.Scene, vf.TerrainSpike):
        for m in ("add_contours", "height_bounds", "layer_primitive_count"):
            assert callable(getattr(cls, m)), (cls, m)
    assert "interval" in vf.Scene.add_contours.__doc__ and "join" in vf.Scene.add_contours.__doc__


def args(levels=None, interval=None, base=0.0, width_px=1.0, rgba=(0, 0, 0, 255), lift=0.0, join="round", bounds=None):
    from vulkan_forge_amd import _overlays as ov
    return ov.contour_args(levels, interval, base, width_px, rgba, lift, join, bounds)


def test_contour_args_levels():
    lv, width, col, lift, join = args(np.array([0.0, 0.5, 2.0]), width_px=3, rgba=(1, 2, 3, 4), lift=0.25, join="none")
    assert lv.dtype == np.float32 and lv.tolist() == [0.0, 0.5, 2.0] and lv.flags.c_contiguous
    assert (width, lift, join) == (3.0, 0.25, 1) and col.dtype == np.uint8 and col.tolist() == [1, 2, 3, 4]
    assert args(np.float32([1.0]))[4] == 0
    with pytest.raises(ValueError, match="exactly one"):
        args()
    with pytest.raises(ValueError, match="exactly one"):
        args(np.float32([1.0]), interval=0.5, bounds=(0, 1))
    with pytest.raises(TypeError, match="float32 or float64"):
        args(np.array([1, 2, 3]))
    with pytest.raises(TypeError, match="float32 or float64"):
        args([1, 2])
    with pytest.raises(ValueError, match="1-D"):
        args(np.zeros((2, 2)))
    with pytest.raises(ValueError, match="1 .. 65536"):
        args(np.zeros(0))
    with pytest.raises(ValueError, match="1 .. 65536"):
        args(np.arange(65537, dtype=np.float64))
    assert len(args(np.arange(65536, dtype=np.float64))[0]) == 65536
    with pytest.raises(ValueError, match="finite"):
        args(np.array([0.0, np.nan]))
    with pytest.raises(ValueError, match="finite"):
        args(np.array([0.0, np.inf]))
    with pytest.raises(ValueError, match="finite as float32"):
        args(np.array([0.0, 1e300]))
    with pytest.raises(ValueError, match="ascending"):
        args(np.array([0.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="ascending"):
        args(np.array([1.0, 0.0]))
    with pytest.raises(ValueError, match="ascending"):
        args(np.array([1.0, 1.0 + 1e-12]))                   # equal once rounded to float32


def test_contour_args_style():
    lv = np.float32([0.0])
    with pytest.raises(ValueError, match="join"):
        args(lv, join="bevel")
    with pytest.raises(TypeError, match="width_px"):
        args(lv, width_px="2")
    with pytest.raises(ValueError, match="width_px"):
        args(lv, width_px=0.0)
    with pytest.raises(ValueError, match="width_px"):
        args(lv, width_px=float("nan"))
    with pytest.raises(TypeError, match="lift"):
        args(lv, lift=True)
    with pytest.raises(ValueError, match="lift"):
        args(lv, lift=float("inf"))
    with pytest.raises(ValueError, match="4 values"):
        args(lv, rgba=(0, 0, 0))
    with pytest.raises(ValueError, match="0..255"):
        args(lv, rgba=(0, 0, 0, 256))
    with pytest.raises(ValueError, match="4-tuple"):
        args(lv, rgba=np.zeros((1, 4), np.uint8))


def test_contour_args_interval():
    lv = args(interval=0.25, bounds=(-0.3, 0.8))[0]
    assert lv.dtype == np.float32 and lv.tolist() == [-0.25, 0.0, 0.25, 0.5, 0.75]
    assert args(interval=0.25, base=0.05, bounds=(0.05, 0.55))[0].tolist() == np.float32([0.05, 0.3, 0.55]).tolist()   # both ends included
    # formed in float64, rounded once: float32(base + k * interval), not an accumulated float32 sum
    lv = args(interval=0.1, base=0.0, bounds=(0.0, 100.0))[0]
    assert np.array_equal(lv, (np.arange(0, 1001, dtype=np.float64) * 0.1).astype(np.float32)[:len(lv)]) and len(lv) in (1000, 1001)
    assert len(args(interval=1.0, bounds=(0.0, 65535.0))[0]) == 65536
    with pytest.raises(ValueError, match="more than 65536"):
        args(interval=1.0, bounds=(0.0, 65536.0))
    with pytest.raises(ValueError, match="more than 65536"):
        args(interval=1e-9, bounds=(-1.0, 1.0))
    with pytest.raises(ValueError, match="positive"):
        args(interval=0.0, bounds=(0, 1))
    with pytest.raises(ValueError, match="positive"):
        args(interval=-1.0, bounds=(0, 1))
    with pytest.raises(ValueError, match="positive"):
        args(interval=float("inf"), bounds=(0, 1))
    with pytest.raises(TypeError, match="interval"):
        args(interval="1", bounds=(0, 1))
    with pytest.raises(ValueError, match="base"):
        args(interval=1.0, base=float("nan"), bounds=(0, 1))
    with pytest.raises(ValueError, match="height bounds"):
        args(interval=1.0)
    with pytest.raises(ValueError, match="no finite height"):
        args(interval=1.0, bounds=(float("inf"), float("-inf")))
    with pytest.raises(ValueError, match="no level"):
        args(interval=1.0, base=0.5, bounds=(0.6, 0.9))
    with pytest.raises(ValueError, match="same float32"):
        args(interval=1e-6, bounds=(1000.0, 1000.01))
