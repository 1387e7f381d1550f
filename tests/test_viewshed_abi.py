"""Viewshed analysis without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the
header documents them, the Python methods exist on both classes with the documented signatures, and the argument rules refuse what
they should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_viewshed": ["t", "enable", "observer_xz", "eye_height", "target_height", "radius", "visible_rgba", "hidden_rgba",
                                            "softness", "bias"],
                "vf_terrain_read_viewshed_field": ["t", "seen"],
                "vf_terrain_viewshed_field_device": ["t", "dev_seen", "stream"],
                "vf_terrain_viewshed_info": ["t", "out"],
                "vf_terrain_debug_viewshed_stage": ["t", "repeats", "ms"],
                "vf_terrain_debug_viewshed_scans": ["t", "count"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("VIEWSHED", (("EYE_HEIGHT", "0.05f"), ("TARGET_HEIGHT", "0.0f"), ("SOFTNESS", "0.02f"), ("BIAS", "0.002f"), ("VISIBLE_RGBA", "0x6060FF40u"),
                                   ("HIDDEN_RGBA", "0x00000000u")))
    abi.check_info_struct("vf_viewshed_info", cabi.ViewshedInfo, 4 * 13 + 8)


def test_the_header_documents_the_calls():
    abi.check_header_documents("viewshed analysis: a line-of-sight field", list(ENTRY_POINTS)[:4],
                               ("DESIGN.md 4l", "VF_ERR_INVALID", "whether or not the viewshed is enabled", "NULL: the context's stream", "One observer per handle"))


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    out = np.zeros(4, np.float32)
    xz, col = (ctypes.c_float * 2)(0.0, 0.0), (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    abi.check_null_refusals([("vf_terrain_set_viewshed", (1, xz, 0.05, 0.0, 0.0, col, col, 0.02, 0.002)),
                             ("vf_terrain_read_viewshed_field", (out.ctypes.data,)),
                             ("vf_terrain_viewshed_field_device", (None, None)),
                             ("vf_terrain_viewshed_info", (ctypes.byref(cabi.ViewshedInfo()),)),
                             ("vf_terrain_debug_viewshed_stage", (1, (ctypes.c_float * 2)())),
                             ("vf_terrain_debug_viewshed_scans", (ctypes.byref(ctypes.c_uint32()),))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "set_viewshed": r"set_viewshed\(self: [\w.]+, observer: object, \*, enabled: object = True, eye_height: object = 0.05\d*, "
                        r"target_height: object = 0.0, radius: object = None, visible_rgba: object = \(64, 255, 96, 96\), "
                        r"hidden_rgba: object = \(0, 0, 0, 0\), softness: object = 0.019\d+, bias: object = 0.002\d*\) -> None",
        "clear_viewshed": r"clear_viewshed\(self: [\w.]+\) -> None",
        "viewshed_field": r"viewshed_field\(self: [\w.]+\) -> numpy",
        "viewshed_info": r"viewshed_info\(self: [\w.]+\) -> object"})


def test_argument_rules():
    from vulkan_forge_amd._viewshed import DEFAULTS, viewshed_args, viewshed_info
    assert DEFAULTS == {"eye_height": 0.05, "target_height": 0.0, "radius": None, "visible_rgba": (64, 255, 96, 96), "hidden_rgba": (0, 0, 0, 0),
                        "softness": 0.02, "bias": 0.002}
    assert viewshed_args((0.5, -1)) == (1, 0.5, -1.0, 0.05, 0.0, 0.0, (64, 255, 96, 96), (0, 0, 0, 0), 0.02, 0.002)
    assert viewshed_args(np.array([1, 2], np.float32), False, 0, np.float32(2.0), 3, [1, 2, 3, 4], np.array([5, 6, 7, 8], np.uint8), 1, 0) \
        == (0, 1.0, 2.0, 0.0, 2.0, 3.0, (1, 2, 3, 4), (5, 6, 7, 8), 1.0, 0.0)
    ok = dict(DEFAULTS)
    for name, bad, exc, msg in (("eye_height", -0.01, ValueError, "eye_height must be >= 0"), ("target_height", -1, ValueError, "target_height must be >= 0"),
                                ("radius", 0.0, ValueError, "radius must be None or > 0"), ("radius", -2.0, ValueError, "radius must be None or > 0"),
                                ("softness", 0.0, ValueError, "softness must be > 0"), ("bias", -1e-9, ValueError, "bias must be >= 0"),
                                ("visible_rgba", (1, 2, 3), ValueError, "visible_rgba must be 4 ints"), ("hidden_rgba", (1, 2, 3, 256), ValueError, "hidden_rgba must be 4 ints"),
                                ("hidden_rgba", (1, 2, 3, -1), ValueError, "hidden_rgba must be 4 ints"), ("visible_rgba", (1, 2, 3, 4.5), TypeError, "visible_rgba must be 4 ints"),
                                ("visible_rgba", 7, TypeError, "visible_rgba must be 4 ints"), ("softness", "soft", TypeError, "softness must be a number")):
        with pytest.raises(exc, match=msg):
            viewshed_args((0.0, 0.0), True, **{**ok, name: bad})
    for name in ("eye_height", "target_height", "radius", "softness", "bias"):
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="must be finite"):
                viewshed_args((0.0, 0.0), True, **{**ok, name: bad})
    for bad in ((float("nan"), 0.0), (0.0, float("-inf"))):
        with pytest.raises(ValueError, match="must be finite"):
            viewshed_args(bad)
    with pytest.raises(ValueError, match=r"observer must be \(x, z\)"):
        viewshed_args((0.0, 0.0, 0.0))
    with pytest.raises(TypeError, match=r"observer must be \(x, z\)"):
        viewshed_args(3.0)
    with pytest.raises(TypeError, match="enabled must be a bool"):
        viewshed_args((0.0, 0.0), "yes")
    d = viewshed_info(1, 1, (3, 4), (0.5, 0.25, -0.5), 0.3, 0.05, 0.0, 0.0, 0.02, 0.002, (64, 255, 96, 96), (0, 0, 0, 0))
    assert d == {"enabled": True, "vertex": (3, 4), "observer_xyz": (0.5, 0.25, -0.5), "eye_y": 0.3, "eye_height": 0.05, "target_height": 0.0,
                 "radius": None, "visible_rgba": (64, 255, 96, 96), "hidden_rgba": (0, 0, 0, 0), "softness": 0.02, "bias": 0.002}
    d = viewshed_info(0, 0, (0, 0), (0.0, 0.0, 0.0), 0.0, 0.05, 0.0, 2.5, 0.02, 0.002, (1, 2, 3, 4), (5, 6, 7, 8))
    assert d["enabled"] is False and d["vertex"] is None and d["observer_xyz"] is None and d["eye_y"] is None and d["radius"] == 2.5
