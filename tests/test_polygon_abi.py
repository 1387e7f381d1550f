"""vf_terrain_add_polygons (include/vf_hip.h) is declared, listed in cabi.SYMBOLS, exported by libvf_hip.so, reported through the
package, and refuses arguments that need no device to check (no GPU needed)."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_add_polygons_is_declared_listed_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vf_hip.h")).read(), flags=re.S)
    sys.path.insert(0, ROOT)
    from vulkan_forge_amd import cabi
    lib = ctypes.CDLL(cabi.DEFAULT_LIB)
    assert re.search(r"\bvf_terrain_add_polygons\s*\(", src)
    assert "vf_terrain_add_polygons" in cabi.SYMBOLS and "vf_terrain_add_polygons" in cabi._PROTOS
    assert hasattr(lib, "vf_terrain_add_polygons")
    import vulkan_forge as vf
    assert "pack_polygons" in vf.__all__ and vf.pack_polygons is vf.pack_polygons
    assert hasattr(vf.Scene, "add_polygons") and hasattr(vf.TerrainSpike, "add_polygons")


def test_add_polygons_refuses_bad_arguments_without_a_device():
    sys.path.insert(0, ROOT)
    from vulkan_forge_amd import cabi
    lib = cabi.load()
    xyz = np.zeros(9, np.float32)
    rings = np.array([0, 3], np.uint32)
    feats = np.array([0, 1], np.uint32)
    col = ctypes.cast((ctypes.c_uint8 * 4)(255, 255, 255, 255), ctypes.c_void_p)
    call = lib.vf_terrain_add_polygons
    assert call(None, xyz.ctypes.data, rings.ctypes.data, 1, feats.ctypes.data, 1, None, col, None, 1.0, 0, None) == cabi.VF_ERR_INVALID
    assert call(None, xyz.ctypes.data, None, 1, feats.ctypes.data, 1, None, col, None, 1.0, 0, None) == cabi.VF_ERR_INVALID
