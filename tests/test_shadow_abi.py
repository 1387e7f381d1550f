"""Cast shadows without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the Python
methods exist on both classes with the documented signatures, and the argument rules refuse what they should."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["vf_terrain_set_shadows", "vf_terrain_read_shadow_field", "vf_terrain_shadow_field_device", "vf_terrain_debug_shadow_stage",
         "vf_terrain_debug_shadow_scans"]


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    src = open(os.path.join(ROOT, "include", "vf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(cabi.DEFAULT_LIB)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), f"{n} is not declared in include/vf_hip.h"
        assert n in cabi.SYMBOLS and hasattr(lib, n), n
    proto = {n: re.search(n + r"\s*\(([^)]*)\)", src).group(1) for n in NAMES}
    names = {n: [re.sub(r"\[\d*\]", "", a.split()[-1]).lstrip("*") for a in proto[n].split(",")] for n in NAMES}
    assert names["vf_terrain_set_shadows"] == ["t", "enable", "strength", "softness", "bias"]
    assert names["vf_terrain_read_shadow_field"] == ["t", "lit"]
    assert names["vf_terrain_shadow_field_device"] == ["t", "dev_lit", "stream"]
    assert names["vf_terrain_debug_shadow_stage"] == ["t", "repeats", "ms"]
    loaded = cabi.load()
    assert len(loaded.vf_terrain_set_shadows.argtypes) == 5 and len(loaded.vf_terrain_read_shadow_field.argtypes) == 2
    assert len(loaded.vf_terrain_shadow_field_device.argtypes) == 3 and len(loaded.vf_terrain_debug_shadow_stage.argtypes) == 3
    for k, v in (("STRENGTH", 0.7), ("SOFTNESS", 0.02), ("BIAS", 0.002)):
        assert re.search(rf"#define VF_SHADOW_{k} {v}f\b", src), k


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    lib = cabi.load()
    out = np.zeros(4, np.float32)
    ms = (ctypes.c_float * 2)()
    count = ctypes.c_uint32()
    assert lib.vf_terrain_set_shadows(None, 1, 0.7, 0.02, 0.002) == cabi.VF_ERR_INVALID
    assert lib.vf_terrain_read_shadow_field(None, out.ctypes.data) == cabi.VF_ERR_INVALID
    assert lib.vf_terrain_shadow_field_device(None, None, None) == cabi.VF_ERR_INVALID
    assert lib.vf_terrain_debug_shadow_stage(None, 1, ms) == cabi.VF_ERR_INVALID
    assert lib.vf_terrain_debug_shadow_scans(None, ctypes.byref(count)) == cabi.VF_ERR_INVALID


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    import vulkan_forge
    import vulkan_forge_amd
    for pkg in (vulkan_forge, vulkan_forge_amd):
        T = getattr(pkg, cls)
        doc = T.set_shadows.__doc__
        F = r"(float|typing\.SupportsFloat \| typing\.SupportsIndex)"
        assert re.search(rf"set_shadows\(self: [\w.]+, enabled: bool = True, \*, strength: {F} = 0.69\d+, softness: {F} = 0.019\d+, bias: {F} = 0.002\d*\) -> None", doc), doc
        assert re.search(r"shadow_field\(self: [\w.]+\) -> numpy", T.shadow_field.__doc__), T.shadow_field.__doc__
        assert re.search(rf"set_sun\(self: [\w.]+, elevation_deg: {F}, azimuth_deg: {F}\) -> None", T.set_sun.__doc__), T.set_sun.__doc__
        assert re.search(rf"set_exposure\(self: [\w.]+, exposure: {F}\) -> None", T.set_exposure.__doc__), T.set_exposure.__doc__


def test_argument_rules():
    from vulkan_forge_amd._shadows import DEFAULTS, shadow_args
    assert DEFAULTS == {"strength": 0.7, "softness": 0.02, "bias": 0.002}
    assert shadow_args(True, **DEFAULTS) == (1, 0.7, 0.02, 0.002)
    assert shadow_args(False, 0, 1, 0) == (0, 0.0, 1.0, 0.0)
    assert shadow_args(True, np.float32(1.0), np.float64(0.5), 0.0) == (1, 1.0, 0.5, 0.0)
    with pytest.raises(ValueError, match=r"strength must lie in \[0, 1\]"):
        shadow_args(True, 1.01, 0.02, 0.002)
    with pytest.raises(ValueError, match=r"strength must lie in \[0, 1\]"):
        shadow_args(True, -0.1, 0.02, 0.002)
    with pytest.raises(ValueError, match="softness must be > 0"):
        shadow_args(True, 0.7, 0.0, 0.002)
    with pytest.raises(ValueError, match="bias must be >= 0"):
        shadow_args(True, 0.7, 0.02, -1e-9)
    for k in range(3):
        for bad in (float("nan"), float("inf")):
            a = [0.7, 0.02, 0.002]
            a[k] = bad
            with pytest.raises(ValueError, match="must be finite"):
                shadow_args(True, *a)
    with pytest.raises(TypeError, match="strength must be a number"):
        shadow_args(True, "dark", 0.02, 0.002)
    with pytest.raises(TypeError, match="enabled must be a bool"):
        shadow_args("yes", 0.7, 0.02, 0.002)
