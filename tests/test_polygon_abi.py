"""vf_terrain_add_polygons (include/vf_hip.h) is declared, listed in cabi.SYMBOLS, exported by libvf_hip.so, reported through the
package, and refuses arguments that need no device to check (no GPU needed)."""
import ctypes

import numpy as np

import abi_support as abi


def test_add_polygons_is_declared_listed_exported_and_bound():
    abi.check_entry_points({"vf_terrain_add_polygons": ["t", "xyz", "ring_offsets", "nrings", "feature_offsets", "nfeatures", "fill_rgba", "default_fill",
                                                        "line_rgba", "line_width_px", "drape", "layer_id"]})
    import vulkan_forge as vf
    assert "pack_polygons" in vf.__all__ and vf.pack_polygons is vf.pack_polygons
    assert hasattr(vf.Scene, "add_polygons") and hasattr(vf.TerrainSpike, "add_polygons")


def test_add_polygons_refuses_bad_arguments_without_a_device():
    xyz = np.zeros(9, np.float32)
    rings = np.array([0, 3], np.uint32)
    feats = np.array([0, 1], np.uint32)
    col = ctypes.cast((ctypes.c_uint8 * 4)(255, 255, 255, 255), ctypes.c_void_p)
    abi.check_null_refusals([("vf_terrain_add_polygons", (xyz.ctypes.data, rings.ctypes.data, 1, feats.ctypes.data, 1, None, col, None, 1.0, 0, None)),
                             ("vf_terrain_add_polygons", (xyz.ctypes.data, None, 1, feats.ctypes.data, 1, None, col, None, 1.0, 0, None))])
