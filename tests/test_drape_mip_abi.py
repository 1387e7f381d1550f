"""The drape's mip pyramid without a device: the header, cabi's tables and the library agree on the three new entry
points and constants, the Python methods exist on both classes with the documented signatures, and the argument rules refuse what
they should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_drape_mips": ["t", "enabled", "bias"],
                "vf_terrain_drape_mip_info": ["t", "enabled", "levels", "bias", "bytes", "builds"],
                "vf_terrain_read_drape_level": ["t", "level", "out", "w", "h"],
                "vf_terrain_debug_drape_mip_build": ["t", "repeats", "ms"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import _drape, cabi
    assert "716 MB" in abi.header_text()                      # the pyramid's memory at the size limit is stated
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("DRAPE_MIP", (("BIAS_MAX", "16.0f"), ("LEVELS_MAX", "15")))
    assert cabi.VF_DRAPE_MIP_BIAS_MAX == 16.0 and cabi.VF_DRAPE_MIP_LEVELS_MAX == 15
    assert (_drape.MIP_BIAS_MAX, _drape.MIP_LEVELS_MAX) == (16.0, 15)


def test_null_arguments_are_refused_without_a_device():
    w = ctypes.c_uint32()
    abi.check_null_refusals([("vf_terrain_set_drape_mips", (1, 0.0)),
                             ("vf_terrain_drape_mip_info", (None, ctypes.byref(w), None, None, None)),
                             ("vf_terrain_read_drape_level", (1, None, ctypes.byref(w), ctypes.byref(w))),
                             ("vf_terrain_debug_drape_mip_build", (1, None))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    A = r"(object|typing\.Any)"
    abi.check_method_docs(cls, {
        "set_drape_mipmaps": rf"set_drape_mipmaps\(self: [\w.]+, enabled: {A} = True, \*, bias: {A} = 0.0\) -> None",
        "drape_mip_info": r"drape_mip_info\(self: [\w.]+\) -> ",
        "read_drape_level": rf"read_drape_level\(self: [\w.]+, level: {A}\) -> "},
        cabi_methods=("set_drape_mipmaps", "drape_mip_info", "drape_mip_builds", "read_drape_level", "drape_mip_build_stage"))


def test_argument_rules():
    from vulkan_forge_amd._drape import MIP_DEFAULTS, mip_info, mip_level, mip_params, mip_sizes
    assert MIP_DEFAULTS == {"enabled": True, "bias": 0.0}
    assert mip_params() == (1, 0.0) and mip_params(False, bias=-16) == (0, -16.0) and mip_params(np.bool_(True), np.float32(1.5)) == (1, 1.5)
    assert mip_params(1, 16.0) == (1, 16.0)
    nan, inf = float("nan"), float("inf")
    for bad in (16.0001, -16.5, 1e30):
        with pytest.raises(ValueError, match=r"bias must lie in \[-16, 16\]"):
            mip_params(True, bad)
    for bad in (nan, inf, -inf):
        with pytest.raises(ValueError, match="bias must be finite"):
            mip_params(True, bad)
    with pytest.raises(TypeError, match="bias must be a number"):
        mip_params(True, "sharp")
    for bad in ("yes", None, 1.0):
        with pytest.raises(TypeError, match="enabled must be a bool"):
            mip_params(bad)
    assert mip_sizes(37, 53) == [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4), (2, 2), (1, 1)]
    assert mip_sizes(1, 1) == [(1, 1)] and len(mip_sizes(16384, 16384)) == 15 and len(mip_sizes(16384, 2)) == 15
    assert mip_sizes(5, 1) == [(5, 1), (3, 1), (2, 1), (1, 1)]
    assert mip_level(1, 7) == 1 and mip_level(np.int64(6), 7) == 6
    for bad, levels in ((0, 7), (7, 7), (-1, 7), (1, 1), (1, 0)):
        with pytest.raises(ValueError, match="level"):
            mip_level(bad, levels)
    for bad in (1.0, True, "1"):
        with pytest.raises(TypeError, match="level must be an int"):
            mip_level(bad, 7)
    assert mip_info(False, 0, 0.0, 0, 3, 37, 53) is None
    assert mip_info(True, 0, 1.5, 0, 0, 0, 0) == {"levels": 0, "sizes": [], "bias": 1.5, "bytes": 0, "builds": 0}
    assert mip_info(True, 7, 0.0, 4560, 2, 37, 53) == {"levels": 7, "sizes": mip_sizes(37, 53), "bias": 0.0, "bytes": 4560, "builds": 2}
