"""Cast shadows without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the Python
methods exist on both classes with the documented signatures, and the argument rules refuse what they should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_shadows": ["t", "enable", "strength", "softness", "bias"],
                "vf_terrain_read_shadow_field": ["t", "lit"],
                "vf_terrain_shadow_field_device": ["t", "dev_lit", "stream"],
                "vf_terrain_debug_shadow_stage": ["t", "repeats", "ms"],
                "vf_terrain_debug_shadow_scans": ["t", "count"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("SHADOW", (("STRENGTH", "0.7f"), ("SOFTNESS", "0.02f"), ("BIAS", "0.002f")))


def test_null_handles_are_refused_without_a_device():
    out = np.zeros(4, np.float32)
    abi.check_null_refusals([("vf_terrain_set_shadows", (1, 0.7, 0.02, 0.002)),
                             ("vf_terrain_read_shadow_field", (out.ctypes.data,)),
                             ("vf_terrain_shadow_field_device", (None, None)),
                             ("vf_terrain_debug_shadow_stage", (1, (ctypes.c_float * 2)())),
                             ("vf_terrain_debug_shadow_scans", (ctypes.byref(ctypes.c_uint32()),))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    F = r"(float|typing\.SupportsFloat \| typing\.SupportsIndex)"
    abi.check_method_docs(cls, {
        "set_shadows": rf"set_shadows\(self: [\w.]+, enabled: bool = True, \*, strength: {F} = 0.69\d+, softness: {F} = 0.019\d+, bias: {F} = 0.002\d*\) -> None",
        "shadow_field": r"shadow_field\(self: [\w.]+\) -> numpy",
        "set_sun": rf"set_sun\(self: [\w.]+, elevation_deg: {F}, azimuth_deg: {F}\) -> None",
        "set_exposure": rf"set_exposure\(self: [\w.]+, exposure: {F}\) -> None"})


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
