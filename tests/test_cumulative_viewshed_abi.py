"""Cumulative viewsheds without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the
header documents them, the Python methods exist on both classes with the documented signatures, and the argument rules refuse what
they should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_cumulative_viewshed": ["t", "enable", "observers_xz", "count", "eye_height", "target_height", "radius", "high_rgba",
                                                       "low_rgba", "softness", "bias"],
                "vf_terrain_read_cumulative_viewshed_field": ["t", "count"],
                "vf_terrain_cumulative_viewshed_field_device": ["t", "dev_count", "stream"],
                "vf_terrain_cumulative_viewshed_info": ["t", "out"],
                "vf_terrain_read_cumulative_viewshed_vertices": ["t", "vertices"],
                "vf_terrain_debug_cumulative_viewshed_batch": ["t", "batch"],
                "vf_terrain_debug_cumulative_viewshed_scans": ["t", "count"],
                "vf_terrain_debug_cumulative_viewshed_stage": ["t", "repeats", "ms"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("CUMULATIVE_VIEWSHED", (("MAX_OBSERVERS", "65535u"), ("HIGH_RGBA", "0xA060FF40u"), ("LOW_RGBA", "0x00000000u")))
    assert 0xA060FF40 == 64 | 255 << 8 | 96 << 16 | 160 << 24
    abi.check_info_struct("vf_cumulative_viewshed_info", cabi.CumulativeViewshedInfo, 4 * 8 + 8)


def test_the_header_documents_the_calls():
    abi.check_header_documents("cumulative viewsheds: how many of N observers see each vertex", list(ENTRY_POINTS)[:5],
                               ("DESIGN.md 4m", "VF_ERR_INVALID", "whether or not the cumulative viewshed is enabled", "NULL: the context's", "1 <= count <= 65535",
                                "rint(seen * 65536)", "Many observers per handle"))


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    out = np.zeros(4, np.float32)
    xz, col = np.zeros((2, 2), np.float32), (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    abi.check_null_refusals([("vf_terrain_set_cumulative_viewshed", (1, xz.ctypes.data, 2, 0.05, 0.0, 0.0, col, col, 0.02, 0.002)),
                             ("vf_terrain_read_cumulative_viewshed_field", (out.ctypes.data,)),
                             ("vf_terrain_cumulative_viewshed_field_device", (None, None)),
                             ("vf_terrain_cumulative_viewshed_info", (ctypes.byref(cabi.CumulativeViewshedInfo()),)),
                             ("vf_terrain_read_cumulative_viewshed_vertices", (out.ctypes.data,)),
                             ("vf_terrain_debug_cumulative_viewshed_batch", (4,)),
                             ("vf_terrain_debug_cumulative_viewshed_scans", (ctypes.byref(ctypes.c_uint32()),)),
                             ("vf_terrain_debug_cumulative_viewshed_stage", (1, ctypes.byref(ctypes.c_float())))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "set_cumulative_viewshed": r"set_cumulative_viewshed\(self: [\w.]+, observers: object, \*, enabled: object = True, eye_height: object = 0.05\d*, "
                                   r"target_height: object = 0.0, radius: object = None, high_rgba: object = \(64, 255, 96, 160\), "
                                   r"low_rgba: object = \(0, 0, 0, 0\), softness: object = 0.019\d+, bias: object = 0.002\d*\) -> None",
        "clear_cumulative_viewshed": r"clear_cumulative_viewshed\(self: [\w.]+\) -> None",
        "cumulative_viewshed_field": r"cumulative_viewshed_field\(self: [\w.]+\) -> numpy",
        "cumulative_viewshed_info": r"cumulative_viewshed_info\(self: [\w.]+\) -> object"},
        cabi_methods=("set_cumulative_viewshed", "clear_cumulative_viewshed", "cumulative_viewshed_field", "cumulative_viewshed_info"))


def test_argument_rules():
    from vulkan_forge_amd._cumulative_viewshed import DEFAULTS, MAX_OBSERVERS, cumulative_viewshed_args, cumulative_viewshed_info
    assert MAX_OBSERVERS == 65535
    assert DEFAULTS == {"eye_height": 0.05, "target_height": 0.0, "radius": None, "high_rgba": (64, 255, 96, 160), "low_rgba": (0, 0, 0, 0),
                        "softness": 0.02, "bias": 0.002}
    a = cumulative_viewshed_args([(0.5, -1), (2, 3)])
    assert a[0] == 1 and a[2:] == (0.05, 0.0, 0.0, (64, 255, 96, 160), (0, 0, 0, 0), 0.02, 0.002)
    assert a[1].dtype == np.float32 and a[1].shape == (2, 2) and a[1].flags.c_contiguous and a[1].tolist() == [[0.5, -1.0], [2.0, 3.0]]
    a = cumulative_viewshed_args(np.arange(12, dtype=np.float64).reshape(2, 6)[:, ::3], False, 0, np.float32(2.0), 3, [1, 2, 3, 4],
                                 np.array([5, 6, 7, 8], np.uint8), 1, 0)
    assert a[0] == 0 and a[1].tolist() == [[0.0, 3.0], [6.0, 9.0]] and a[1].flags.c_contiguous
    assert a[2:] == (0.0, 2.0, 3.0, (1, 2, 3, 4), (5, 6, 7, 8), 1.0, 0.0)
    assert cumulative_viewshed_args(np.zeros((MAX_OBSERVERS, 2)))[1].shape == (MAX_OBSERVERS, 2)
    ok = dict(DEFAULTS)
    one = [(0.0, 0.0)]
    for name, bad, exc, msg in (("eye_height", -0.01, ValueError, "eye_height must be >= 0"), ("target_height", -1, ValueError, "target_height must be >= 0"),
                                ("radius", 0.0, ValueError, "radius must be None or > 0"), ("radius", -2.0, ValueError, "radius must be None or > 0"),
                                ("softness", 0.0, ValueError, "softness must be > 0"), ("bias", -1e-9, ValueError, "bias must be >= 0"),
                                ("high_rgba", (1, 2, 3), ValueError, "high_rgba must be 4 ints"), ("low_rgba", (1, 2, 3, 256), ValueError, "low_rgba must be 4 ints"),
                                ("low_rgba", (1, 2, 3, -1), ValueError, "low_rgba must be 4 ints"), ("high_rgba", (1, 2, 3, 4.5), TypeError, "high_rgba must be 4 ints"),
                                ("high_rgba", 7, TypeError, "high_rgba must be 4 ints"), ("softness", "soft", TypeError, "softness must be a number")):
        with pytest.raises(exc, match=msg):
            cumulative_viewshed_args(one, True, **{**ok, name: bad})
    for name in ("eye_height", "target_height", "radius", "softness", "bias"):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="must be finite"):
                cumulative_viewshed_args(one, True, **{**ok, name: bad})
    for bad in ([(float("nan"), 0.0)], [(0.0, 0.0), (0.0, float("-inf"))]):
        with pytest.raises(ValueError, match="observers must be finite"):
            cumulative_viewshed_args(bad)
    for bad in ((0.0, 0.0), [(0.0, 0.0, 0.0)], np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"observers must be \(N, 2\)"):
            cumulative_viewshed_args(bad)
    for bad in (np.zeros((0, 2)), np.zeros((MAX_OBSERVERS + 1, 2))):
        with pytest.raises(ValueError, match="observers must hold 1 to 65535 rows"):
            cumulative_viewshed_args(bad)
    for bad in ([("a", "b")], [(None, 1.0)], [(1j, 0.0)]):
        with pytest.raises(TypeError, match=r"observers must be \(N, 2\) numbers"):
            cumulative_viewshed_args(bad)
    with pytest.raises(TypeError, match="enabled must be a bool"):
        cumulative_viewshed_args(one, "yes")
    d = cumulative_viewshed_info(1, 2, 2, np.array([[3, 4], [5, 6]], np.uint32), 0.05, 0.0, 0.0, 0.02, 0.002, (64, 255, 96, 160), (0, 0, 0, 0))
    vertices = d.pop("vertices")
    assert vertices.dtype == np.uint32 and vertices.tolist() == [[3, 4], [5, 6]]
    assert d == {"enabled": True, "observers": 2, "batch": 2, "eye_height": 0.05, "target_height": 0.0, "radius": None,
                 "high_rgba": (64, 255, 96, 160), "low_rgba": (0, 0, 0, 0), "softness": 0.02, "bias": 0.002}
    d = cumulative_viewshed_info(0, 0, 0, None, 0.05, 0.0, 2.5, 0.02, 0.002, (1, 2, 3, 4), (5, 6, 7, 8))
    assert d["enabled"] is False and d["vertices"] is None and d["observers"] == 0 and d["radius"] == 2.5
