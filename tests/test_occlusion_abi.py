"""vf_terrain_set_layer_occlusion (include/vf_hip.h) is declared, listed in cabi.SYMBOLS with its ctypes signature, exported by
libvf_hip.so, and refuses what needs no device to check; the Python argument rules of occlude / depth_bias (no GPU needed)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import abi_support as abi
from support import ROOT

_spec = importlib.util.spec_from_file_location("vf_overlay_rules", os.path.join(ROOT, "vulkan_forge_amd", "_overlays.py"))
ov = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ov)


def test_set_layer_occlusion_is_declared_listed_and_exported():
    from vulkan_forge_amd import cabi
    abi.check_entry_points({"vf_terrain_set_layer_occlusion": ["t", "layer_id", "occlude", "depth_bias"]})
    assert re.search(r"int\s+vf_terrain_set_layer_occlusion\s*\(\s*vf_terrain\s*\*\s*t\s*,\s*uint32_t\s+layer_id\s*,\s*int\s+occlude\s*,"
                     r"\s*float\s+depth_bias\s*\)\s*;", abi.code())
    abi.check_defines("OCCLUSION", (("DEPTH_BIAS", "1e-2f"),))
    restype, argtypes = cabi._PROTOS["vf_terrain_set_layer_occlusion"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_float]
    abi.check_null_refusals([("vf_terrain_set_layer_occlusion", (0, 1, 0.01))])


def test_occlusion_argument_rules():
    assert ov.occlusion_args(False, 1e-2) == (False, 1e-2)
    assert ov.occlusion_args(np.bool_(True), 0) == (True, 0.0)
    assert ov.occlusion_args(True, np.float32(0.5)) == (True, 0.5)
    with pytest.raises(TypeError, match="occlude must be a bool"):
        ov.occlusion_args(1, 0.01)
    with pytest.raises(TypeError, match="depth_bias must be a number"):
        ov.occlusion_args(True, "0.01")
    with pytest.raises(TypeError, match="depth_bias must be a number"):
        ov.occlusion_args(True, True)
    for bad in (-1e-3, float("nan"), float("inf"), 1e300):
        with pytest.raises(ValueError, match="depth_bias must be a finite number >= 0"):
            ov.occlusion_args(True, bad)


def test_the_methods_take_occlusion_arguments():
    pytest.importorskip("vulkan_forge_amd._vulkan_forge")
    import vulkan_forge as vf
    for cls in (vf.Scene, vf.TerrainSpike):
        assert hasattr(cls, "set_layer_occlusion")
        for meth in ("add_points", "add_lines"):
            assert "occlude" in getattr(cls, meth).__doc__ and "depth_bias" in getattr(cls, meth).__doc__
