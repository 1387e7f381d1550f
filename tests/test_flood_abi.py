"""Flood analysis without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the header
documents them, the Python methods exist on both classes with the documented signatures, and the argument rules refuse what they
should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_flood": ["t", "enable", "level", "mode", "seeds_xz", "count", "shallow_rgba", "deep_rgba", "depth_full"],
                "vf_terrain_clear_flood": ["t"],
                "vf_terrain_read_flood_field": ["t", "depth"],
                "vf_terrain_flood_field_device": ["t", "dev_depth", "stream"],
                "vf_terrain_flood_info": ["t", "out"],
                "vf_terrain_read_flood_seeds": ["t", "vertices"],
                "vf_terrain_debug_flood_scans": ["t", "count"],
                "vf_terrain_debug_flood_group": ["t", "group"],
                "vf_terrain_debug_flood_stage": ["t", "repeats", "ms"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("FLOOD", (("EVERYWHERE", "0"), ("EDGES", "1"), ("SEEDS", "2"), ("MAX_SEEDS", "65535u"), ("SHALLOW_RGBA", "0x80E0B060u"),
                                ("DEEP_RGBA", "0xE0A04010u"), ("DEPTH_FULL", "0.1f")))
    assert 0x80E0B060 == 96 | 176 << 8 | 224 << 16 | 128 << 24 and 0xE0A04010 == 16 | 64 << 8 | 160 << 16 | 224 << 24
    abi.check_info_struct("vf_flood_info", cabi.FloodInfo, 4 * 6 + 8 + 4 * 5)


def test_the_header_documents_the_calls():
    abi.check_header_documents("flood analysis: what is under water at a level", list(ENTRY_POINTS)[:6],
                               ("DESIGN.md 4s", "VF_ERR_INVALID", "whether or not the flood is enabled", "NULL: the context's", "1 <= count <= 65535",
                                "4-connected", "least fixpoint", "before exaggeration", "vf_terrain_add_contours", "Whole-frame handles only",
                                "survives height uploads", "allocates and launches nothing"))


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    out = np.zeros(4, np.float32)
    xz, col = np.zeros((2, 2), np.float32), (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    abi.check_null_refusals([("vf_terrain_set_flood", (1, 0.0, 2, xz.ctypes.data, 2, col, col, 0.1)),
                             ("vf_terrain_clear_flood", ()),
                             ("vf_terrain_read_flood_field", (out.ctypes.data,)),
                             ("vf_terrain_flood_field_device", (None, None)),
                             ("vf_terrain_flood_info", (ctypes.byref(cabi.FloodInfo()),)),
                             ("vf_terrain_read_flood_seeds", (out.ctypes.data,)),
                             ("vf_terrain_debug_flood_scans", (ctypes.byref(ctypes.c_uint32()),)),
                             ("vf_terrain_debug_flood_group", (4,)),
                             ("vf_terrain_debug_flood_stage", (1, (ctypes.c_float * 2)()))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "set_flood": r"set_flood\(self: [\w.]+, level: object, seeds: object = None, \*, enabled: object = True, "
                     r"shallow_rgba: object = \(96, 176, 224, 128\), deep_rgba: object = \(16, 64, 160, 224\), "
                     r"depth_full: object = 0.100\d*\) -> None",
        "clear_flood": r"clear_flood\(self: [\w.]+\) -> None",
        "flood_field": r"flood_field\(self: [\w.]+\) -> numpy",
        "flood_info": r"flood_info\(self: [\w.]+\) -> object"},
        cabi_methods=("set_flood", "clear_flood", "flood_field", "flood_field_device", "flood_info", "flood_scans", "flood_group"))


def test_argument_rules():
    from vulkan_forge_amd._flood import DEFAULTS, EDGES, EVERYWHERE, MAX_SEEDS, MODES, SEEDS, flood_args, flood_info
    assert MAX_SEEDS == 65535 and (EVERYWHERE, EDGES, SEEDS) == (0, 1, 2) and MODES == ("everywhere", "edges", "seeds")
    assert DEFAULTS == {"shallow_rgba": (96, 176, 224, 128), "deep_rgba": (16, 64, 160, 224), "depth_full": 0.1}
    assert flood_args(0.25) == (1, 0.25, EVERYWHERE, None, (96, 176, 224, 128), (16, 64, 160, 224), 0.1)
    assert flood_args(-1, "edges", False, [1, 2, 3, 4], np.array([5, 6, 7, 8], np.uint8), 2) == (0, -1.0, EDGES, None, (1, 2, 3, 4), (5, 6, 7, 8), 2.0)
    a = flood_args(np.float32(0.5), [(0.5, -1), (2, 3)])
    assert a[:3] == (1, 0.5, SEEDS) and a[4:] == ((96, 176, 224, 128), (16, 64, 160, 224), 0.1)
    assert a[3].dtype == np.float32 and a[3].shape == (2, 2) and a[3].flags.c_contiguous and a[3].tolist() == [[0.5, -1.0], [2.0, 3.0]]
    a = flood_args(0, np.arange(12, dtype=np.float64).reshape(2, 6)[:, ::3])
    assert a[3].tolist() == [[0.0, 3.0], [6.0, 9.0]] and a[3].flags.c_contiguous
    assert flood_args(0, np.zeros((MAX_SEEDS, 2)))[3].shape == (MAX_SEEDS, 2)
    for kw, exc, msg in ((dict(depth_full=0.0), ValueError, "depth_full must be > 0"), (dict(depth_full=-1), ValueError, "depth_full must be > 0"),
                         (dict(depth_full="deep"), TypeError, "depth_full must be a number"),
                         (dict(shallow_rgba=(1, 2, 3)), ValueError, "shallow_rgba must be 4 ints"), (dict(deep_rgba=(1, 2, 3, 256)), ValueError, "deep_rgba must be 4 ints"),
                         (dict(deep_rgba=(1, 2, 3, 4.5)), TypeError, "deep_rgba must be 4 ints"), (dict(shallow_rgba=7), TypeError, "shallow_rgba must be 4 ints"),
                         (dict(enabled="yes"), TypeError, "enabled must be a bool")):
        with pytest.raises(exc, match=msg):
            flood_args(0.1, None, **kw)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="level must be finite"):
            flood_args(bad)
        with pytest.raises(ValueError, match="depth_full must be finite"):
            flood_args(0.1, depth_full=bad)
    with pytest.raises(TypeError, match="level must be a number"):
        flood_args("high")
    for bad in ([(float("nan"), 0.0)], [(0.0, 0.0), (0.0, float("-inf"))]):
        with pytest.raises(ValueError, match="seeds must be finite"):
            flood_args(0.1, bad)
    for bad in ((0.0, 0.0), [(0.0, 0.0, 0.0)], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"seeds must be \(N, 2\)"):
            flood_args(0.1, bad)
    for bad in (np.zeros((0, 2)), np.zeros((MAX_SEEDS + 1, 2))):
        with pytest.raises(ValueError, match="seeds must hold 1 to 65535 rows"):
            flood_args(0.1, bad)
    for bad in ([("a", "b")], [(None, 1.0)], [(1j, 0.0)]):
        with pytest.raises(TypeError, match=r'seeds must be None, "edges" or \(N, 2\) numbers'):
            flood_args(0.1, bad)
    for bad in ("coast", "everywhere", ""):
        with pytest.raises(ValueError, match='seeds must be None, "edges"'):
            flood_args(0.1, bad)
    d = flood_info(1, 1, 2, 2, np.array([[3, 4], [5, 6]], np.uint32), 0.25, 0.1, (96, 176, 224, 128), (16, 64, 160, 224), 10, 20, 3, 1, 4)
    vertices = d.pop("vertices")
    assert vertices.dtype == np.uint32 and vertices.tolist() == [[3, 4], [5, 6]]
    assert d == {"enabled": True, "level": 0.25, "mode": "seeds", "seeds": 2, "shallow_rgba": (96, 176, 224, 128), "deep_rgba": (16, 64, 160, 224),
                 "depth_full": pytest.approx(0.1), "flooded_vertices": 10, "wettable_vertices": 20, "passes": 3, "scans": 1, "group": 4}
    d = flood_info(0, 0, 0, 0, None, 0.0, 0.1, (1, 2, 3, 4), (5, 6, 7, 8), 0, 0, 0, 0, 4)
    assert d["enabled"] is False and d["vertices"] is None and d["level"] is None and d["mode"] is None and d["seeds"] == 0
