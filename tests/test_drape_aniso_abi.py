"""Anisotropic filtering of the drape's mip sampling without a device: the header, cabi's tables and the library agree on
the two entry points and the constant, NULL handles are refused, the Python methods exist on both classes of both packages with the
documented signatures, and the argument rule accepts and refuses what it should."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_drape_anisotropy": ["t", "max_anisotropy"], "vf_terrain_drape_anisotropy": ["t", "max_anisotropy"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import _drape, cabi
    abi.check_entry_points(ENTRY_POINTS)
    src = abi.code()
    proto = {n: re.search(n + r"\s*\(([^)]*)\)", src).group(1) for n in ENTRY_POINTS}
    assert re.search(r"vf_terrain \*t, uint32_t max_anisotropy", proto["vf_terrain_set_drape_anisotropy"])
    assert re.search(r"const vf_terrain \*t, uint32_t \*max_anisotropy", proto["vf_terrain_drape_anisotropy"])
    abi.check_defines("DRAPE", (("ANISOTROPY_MAX", "16"),))
    assert cabi.VF_DRAPE_ANISOTROPY_MAX == 16
    assert _drape.ANISOTROPY_MAX == 16 and _drape.ANISOTROPIES == (1, 2, 4, 8, 16)


def test_null_arguments_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    lib = cabi.load()
    a = ctypes.c_uint32(7)
    abi.check_null_refusals([("vf_terrain_set_drape_anisotropy", (4,))])
    assert lib.vf_last_error().decode() == "NULL argument"
    abi.check_null_refusals([("vf_terrain_drape_anisotropy", (ctypes.byref(a),)), ("vf_terrain_drape_anisotropy", (None,))])
    assert a.value == 7


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    from vulkan_forge_amd import cabi
    A = r"(object|typing\.Any)"
    abi.check_method_docs(cls, {
        "set_drape_anisotropy": rf"set_drape_anisotropy\(self: [\w.]+, max_anisotropy: {A} = 1\) -> None",
        "drape_anisotropy": r"drape_anisotropy\(self: [\w.]+\) -> int"},
        cabi_methods=("set_drape_anisotropy", "drape_anisotropy"))
    assert str(inspect.signature(cabi.Terrain.set_drape_anisotropy)) == "(self, max_anisotropy=1)"
    assert str(inspect.signature(cabi.Terrain.drape_anisotropy)) == "(self)"


def test_argument_rules():
    from vulkan_forge_amd._drape import aniso_params
    assert str(inspect.signature(aniso_params)) == "(max_anisotropy=1)"
    assert aniso_params() == 1
    for a in (1, 2, 4, 8, 16):
        for v in (a, np.int64(a), np.uint8(a), np.int32(a)):
            got = aniso_params(v)
            assert got == a and type(got) is int
    for bad in (0, 3, 5, 6, 12, 15, 17, 32, -1, -2, 2 ** 40, np.int64(3)):
        with pytest.raises(ValueError, match=r"max_anisotropy must be 1, 2, 4, 8 or 16"):
            aniso_params(bad)
    for bad in (True, False, np.bool_(True), 2.0, np.float32(4.0), "4", b"4", None, (4,), [2]):
        with pytest.raises(TypeError, match="max_anisotropy must be an int"):
            aniso_params(bad)
