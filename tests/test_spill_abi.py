"""Spill analysis without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the header
documents them, the Python methods exist on both classes with the documented signatures, and the argument rules refuse what they
should."""
import ctypes
import re

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_spill": ["t", "enable", "mode", "seeds_xz", "count", "shallow_rgba", "deep_rgba", "depth_full"],
                "vf_terrain_clear_spill": ["t"],
                "vf_terrain_read_spill_field": ["t", "spill"],
                "vf_terrain_spill_field_device": ["t", "dev_spill", "stream"],
                "vf_terrain_read_sink_depth": ["t", "depth"],
                "vf_terrain_spill_info": ["t", "out"],
                "vf_terrain_read_spill_seeds": ["t", "vertices"],
                "vf_terrain_debug_spill_scans": ["t", "count"],
                "vf_terrain_debug_spill_group": ["t", "group"],
                "vf_terrain_debug_spill_stage": ["t", "repeats", "ms"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("SPILL", (("EDGES", "1"), ("SEEDS", "2"), ("MAX_SEEDS", "65535u"), ("SHALLOW_RGBA", "0x80E0B060u"), ("DEEP_RGBA", "0xE0A04010u"),
                                ("DEPTH_FULL", "0.1f"), ("GROUP_NO_FLAGS", "0x80000000u")))
    src = abi.code()
    assert not re.search(r"#define VF_SPILL_EVERYWHERE", src)  # there is no such mode: its field would be h
    for k in ("EDGES", "SEEDS"):                               # the two modes carry the flood's numbers
        assert re.search(rf"#define VF_SPILL_{k} (\d)", src).group(1) == re.search(rf"#define VF_FLOOD_{k} (\d)", src).group(1)
    abi.check_info_struct("vf_spill_info", cabi.SpillInfo, 4 * 5 + 8 + 4 * 6)


def test_the_header_documents_the_calls():
    abi.check_header_documents("spill analysis: the level the water must reach", list(ENTRY_POINTS)[:7],
                               ("DESIGN.md 4t", "VF_ERR_INVALID", "whether or not the spill is enabled", "NULL: the context's", "1 <= count <= 65535",
                                "4-connected", "greatest fixpoint", "-0 below", "0xFFFFFFFF : 0x80000000", "vf_terrain_set_flood", "Whole-frame handles only",
                                "survives height uploads", "allocates and launches nothing", "+inf where no", "depression-filled"))


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    out = np.zeros(4, np.float32)
    xz, col = np.zeros((2, 2), np.float32), (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    abi.check_null_refusals([("vf_terrain_set_spill", (1, 2, xz.ctypes.data, 2, col, col, 0.1)),
                             ("vf_terrain_clear_spill", ()),
                             ("vf_terrain_read_spill_field", (out.ctypes.data,)),
                             ("vf_terrain_spill_field_device", (None, None)),
                             ("vf_terrain_read_sink_depth", (out.ctypes.data,)),
                             ("vf_terrain_spill_info", (ctypes.byref(cabi.SpillInfo()),)),
                             ("vf_terrain_read_spill_seeds", (out.ctypes.data,)),
                             ("vf_terrain_debug_spill_scans", (ctypes.byref(ctypes.c_uint32()),)),
                             ("vf_terrain_debug_spill_group", (4,)),
                             ("vf_terrain_debug_spill_stage", (1, (ctypes.c_float * 2)()))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "set_spill": r"set_spill\(self: [\w.]+, seeds: object = 'edges', \*, enabled: object = True, "
                     r"shallow_rgba: object = \(96, 176, 224, 128\), deep_rgba: object = \(16, 64, 160, 224\), "
                     r"depth_full: object = 0.100\d*\) -> None",
        "clear_spill": r"clear_spill\(self: [\w.]+\) -> None",
        "spill_field": r"spill_field\(self: [\w.]+\) -> numpy",
        "sink_depth_field": r"sink_depth_field\(self: [\w.]+\) -> numpy",
        "spill_info": r"spill_info\(self: [\w.]+\) -> object"},
        cabi_methods=("set_spill", "clear_spill", "spill_field", "spill_field_device", "sink_depth_field", "spill_info", "spill_scans", "spill_group",
                      "spill_stage"))


def test_argument_rules():
    from vulkan_forge_amd._spill import DEFAULTS, EDGES, MAX_SEEDS, MODES, SEEDS, spill_args, spill_info
    assert MAX_SEEDS == 65535 and (EDGES, SEEDS) == (1, 2) and MODES == {1: "edges", 2: "seeds"}
    assert DEFAULTS == {"shallow_rgba": (96, 176, 224, 128), "deep_rgba": (16, 64, 160, 224), "depth_full": 0.1}
    assert spill_args() == (1, EDGES, None, (96, 176, 224, 128), (16, 64, 160, 224), 0.1)
    assert spill_args("edges", False, [1, 2, 3, 4], np.array([5, 6, 7, 8], np.uint8), 2) == (0, EDGES, None, (1, 2, 3, 4), (5, 6, 7, 8), 2.0)
    a = spill_args([(0.5, -1), (2, 3)])
    assert a[:2] == (1, SEEDS) and a[3:] == ((96, 176, 224, 128), (16, 64, 160, 224), 0.1)
    assert a[2].dtype == np.float32 and a[2].shape == (2, 2) and a[2].flags.c_contiguous and a[2].tolist() == [[0.5, -1.0], [2.0, 3.0]]
    a = spill_args(np.arange(12, dtype=np.float64).reshape(2, 6)[:, ::3])
    assert a[2].tolist() == [[0.0, 3.0], [6.0, 9.0]] and a[2].flags.c_contiguous
    assert spill_args(np.zeros((MAX_SEEDS, 2)))[2].shape == (MAX_SEEDS, 2)
    assert spill_args([(1.0, 2.0), (1.0, 2.0)])[2].shape == (2, 2)          # duplicates are allowed
    for kw, exc, msg in ((dict(depth_full=0.0), ValueError, "depth_full must be > 0"), (dict(depth_full=-1), ValueError, "depth_full must be > 0"),
                         (dict(depth_full="deep"), TypeError, "depth_full must be a number"),
                         (dict(shallow_rgba=(1, 2, 3)), ValueError, "shallow_rgba must be 4 ints"), (dict(deep_rgba=(1, 2, 3, 256)), ValueError, "deep_rgba must be 4 ints"),
                         (dict(deep_rgba=(1, 2, 3, 4.5)), TypeError, "deep_rgba must be 4 ints"), (dict(shallow_rgba=7), TypeError, "shallow_rgba must be 4 ints"),
                         (dict(enabled="yes"), TypeError, "enabled must be a bool")):
        with pytest.raises(exc, match=msg):
            spill_args("edges", **kw)
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="depth_full must be finite"):
            spill_args(depth_full=bad)
    for bad in ([(float("nan"), 0.0)], [(0.0, 0.0), (0.0, float("-inf"))]):
        with pytest.raises(ValueError, match="seeds must be finite"):
            spill_args(bad)
    for bad in ((0.0, 0.0), [(0.0, 0.0, 0.0)], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"seeds must be \(N, 2\)"):
            spill_args(bad)
    for bad in (np.zeros((0, 2)), np.zeros((MAX_SEEDS + 1, 2))):
        with pytest.raises(ValueError, match="seeds must hold 1 to 65535 rows"):
            spill_args(bad)
    for bad in ([("a", "b")], [(None, 1.0)], [(1j, 0.0)]):
        with pytest.raises(TypeError, match=r'seeds must be "edges" or \(N, 2\) numbers'):
            spill_args(bad)
    for bad in ("coast", "everywhere", "", None):              # no `everywhere` mode: its field would be h
        with pytest.raises(ValueError, match='seeds must be "edges"'):
            spill_args(bad)
    d = spill_info(1, 1, 2, 2, np.array([[3, 4], [5, 6]], np.uint32), 0.1, (96, 176, 224, 128), (16, 64, 160, 224), 10, 20, 3, 1, 4, 9)
    vertices = d.pop("vertices")
    assert vertices.dtype == np.uint32 and vertices.tolist() == [[3, 4], [5, 6]]
    assert d == {"enabled": True, "mode": "seeds", "seeds": 2, "shallow_rgba": (96, 176, 224, 128), "deep_rgba": (16, 64, 160, 224),
                 "depth_full": pytest.approx(0.1), "reached_vertices": 10, "sink_vertices": 20, "passes": 3, "scans": 1, "group": 4, "tile_runs": 9}
    d = spill_info(0, 0, 1, 0, None, 0.1, (1, 2, 3, 4), (5, 6, 7, 8), 0, 0, 0, 0, 16, 0)
    assert d["enabled"] is False and d["vertices"] is None and d["mode"] is None and d["seeds"] == 0
