"""Atmospheric haze without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the header
documents them, NULL handles are refused, the Python methods exist on both classes with the documented signatures, and the argument
rules refuse what they should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_haze": ["t", "enable", "density", "rgba", "start", "falloff", "base", "max_opacity", "background"],
                "vf_terrain_clear_haze": ["t"],
                "vf_terrain_haze_info": ["t", "out"],
                "vf_terrain_read_haze_opacity": ["t", "dst"],
                "vf_terrain_haze_opacity_device": ["t", "dev", "stream"],
                "vf_terrain_debug_haze_stage": ["t", "repeats", "ms"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("HAZE", (("RGBA", "0xFFEBD7C8u"),))
    assert 0xFFEBD7C8 == 200 | 215 << 8 | 235 << 16 | 255 << 24
    fields = abi.check_info_struct("vf_haze_info", cabi.HazeInfo, 4 * 10)
    assert fields == ["enabled", "background", "density", "start", "falloff", "base", "max_opacity", "rgba", "has_eye", "eye_y"]


def test_the_header_documents_the_calls():
    abi.check_header_documents("atmospheric haze: a distance and height fog pass", list(ENTRY_POINTS),
                               ("DESIGN.md 4q", "VF_ERR_INVALID", "max_opacity outside\n * [0, 1]", "rgba == NULL", "vf_terrain_render_batch / _batch_host",
                                "the sample size on a supersampled handle", "NULL: the context's stream", "are not hazed", "keep their alpha byte",
                                "does not follow vf_terrain_set_shade_precision", "allocates and launches nothing"))


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    out = np.zeros(4, np.float32)
    col = (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    abi.check_null_refusals([("vf_terrain_set_haze", (1, 0.25, col, 0.0, 0.0, 0.0, 1.0, 0)),
                             ("vf_terrain_clear_haze", ()),
                             ("vf_terrain_haze_info", (ctypes.byref(cabi.HazeInfo()),)),
                             ("vf_terrain_read_haze_opacity", (out.ctypes.data,)),
                             ("vf_terrain_haze_opacity_device", (None, None)),
                             ("vf_terrain_debug_haze_stage", (1, ctypes.byref(ctypes.c_float())))])
    assert b"NULL" in cabi.load().vf_last_error()


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "set_haze": r"set_haze\(self: [\w.]+, density: object, \*, rgba: object = \(200, 215, 235, 255\), start: object = 0.0, "
                    r"falloff: object = None, base: object = 0.0, max_opacity: object = 1.0, background: object = False, "
                    r"enabled: object = True\) -> None",
        "clear_haze": r"clear_haze\(self: [\w.]+\) -> None",
        "haze_info": r"haze_info\(self: [\w.]+\) -> object",
        "haze_opacity": r"haze_opacity\(self: [\w.]+\) -> numpy"},
        cabi_methods=("set_haze", "clear_haze", "haze_info", "haze_opacity", "haze_opacity_device", "haze_stage"))


def test_argument_rules():
    from vulkan_forge_amd._haze import DEFAULTS, haze_args, haze_info
    assert DEFAULTS == {"rgba": (200, 215, 235, 255), "start": 0.0, "falloff": None, "base": 0.0, "max_opacity": 1.0, "background": False}
    assert haze_args(0.25) == (1, 0.25, (200, 215, 235, 255), 0.0, 0.0, 0.0, 1.0, 0)
    assert haze_args(np.float32(0.5), [1, 2, 3, 4], 2, 8, -1.5, 0.75, True, False) == (0, 0.5, (1, 2, 3, 4), 2.0, 8.0, -1.5, 0.75, 1)
    assert haze_args(0, np.array([9, 8, 7, 0], np.uint8), max_opacity=0)[1:3] == (0.0, (9, 8, 7, 0))      # (no haze at all is allowed)
    assert haze_args(1.0, max_opacity=1)[6] == 1.0
    for kw, exc, msg in ((dict(density=-0.1), ValueError, "density must be >= 0"), (dict(density="thick"), TypeError, "density must be a number"),
                         (dict(density=None), TypeError, "density must be a number"), (dict(density=1j), TypeError, "density must be a number"),
                         (dict(start=-1e-9), ValueError, "start must be >= 0"), (dict(start="far"), TypeError, "start must be a number"),
                         (dict(falloff=0.0), ValueError, r"falloff must be None \(uniform haze\) or > 0"),
                         (dict(falloff=-2.0), ValueError, r"falloff must be None \(uniform haze\) or > 0"),
                         (dict(falloff="steep"), TypeError, "falloff must be a number"), (dict(base="sea"), TypeError, "base must be a number"),
                         (dict(max_opacity=1.0001), ValueError, r"max_opacity must lie in \[0, 1\]"),
                         (dict(max_opacity=-0.01), ValueError, r"max_opacity must lie in \[0, 1\]"),
                         (dict(max_opacity=None), TypeError, "max_opacity must be a number"),
                         (dict(rgba=(1, 2, 3)), ValueError, "rgba must be 4 ints"), (dict(rgba=(1, 2, 3, 256)), ValueError, "rgba must be 4 ints"),
                         (dict(rgba=(1, 2, 3, -1)), ValueError, "rgba must be 4 ints"), (dict(rgba=(1, 2, 3, 4.5)), TypeError, "rgba must be 4 ints"),
                         (dict(rgba=7), TypeError, "rgba must be 4 ints"), (dict(rgba=None), TypeError, "rgba must be 4 ints"),
                         (dict(background="sky"), TypeError, "background must be a bool"), (dict(enabled="yes"), TypeError, "enabled must be a bool")):
        with pytest.raises(exc, match=msg):
            haze_args(**{"density": 0.25, **kw})
    for name in ("density", "start", "falloff", "base", "max_opacity"):
        for bad in (float("nan"), float("inf"), float("-inf")):
            with pytest.raises(ValueError, match=f"{name} must be finite"):
                haze_args(**{"density": 0.25, name: bad})
    d = haze_info(1, 1, 0.25, 2.0, 8.0, 0.5, 0.75, (1, 2, 3, 4), 1, 2.5)
    assert d == {"enabled": True, "density": 0.25, "rgba": (1, 2, 3, 4), "start": 2.0, "falloff": 8.0, "base": 0.5, "max_opacity": 0.75,
                 "background": True, "eye_y": 2.5}
    d = haze_info(0, 0, 0.0, 0.0, 0.0, 0.0, 1.0, (200, 215, 235, 255), 0, 0.0)
    assert d["enabled"] is False and d["background"] is False and d["falloff"] is None and d["eye_y"] is None
