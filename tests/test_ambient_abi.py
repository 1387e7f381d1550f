"""Ambient occlusion without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the
Python methods exist on both classes with the documented signatures, and the argument rules refuse what they should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_ambient": ["t", "enable", "strength", "reach", "ndirs", "dirs_xz"],
                "vf_terrain_read_sky_view_field": ["t", "sky"],
                "vf_terrain_sky_view_field_device": ["t", "dev_sky", "stream"],
                "vf_terrain_debug_ambient_stage": ["t", "repeats", "ms"],
                "vf_terrain_debug_ambient_scans": ["t", "count"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("AMBIENT", (("STRENGTH", "0.6f"), ("REACH", "64.0f"), ("DIRECTIONS", "16")))


def test_null_handles_are_refused_without_a_device():
    out = np.zeros(4, np.float32)
    abi.check_null_refusals([("vf_terrain_set_ambient", (1, 0.6, 64.0, 16, None)),
                             ("vf_terrain_read_sky_view_field", (out.ctypes.data,)),
                             ("vf_terrain_sky_view_field_device", (None, None)),
                             ("vf_terrain_debug_ambient_stage", (1, (ctypes.c_float * 2)())),
                             ("vf_terrain_debug_ambient_scans", (ctypes.byref(ctypes.c_uint32()),))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    F = r"(float|typing\.SupportsFloat \| typing\.SupportsIndex)"
    abi.check_method_docs(cls, {
        "set_ambient_occlusion": rf"set_ambient_occlusion\(self: [\w.]+, enabled: bool = True, \*, strength: {F} = 0.60\d+, reach: {F} = 64.0, directions: (object|typing\.Any) = 16\) -> None",
        "sky_view_field": r"sky_view_field\(self: [\w.]+\) -> numpy"},
        cabi_methods=("set_ambient_occlusion", "sky_view_field", "sky_view_field_device"))


def test_the_default_directions():
    from vulkan_forge_amd._ambient import directions
    d = directions(16)
    assert d.shape == (16, 2) and d.dtype == np.float32
    assert d[0].tolist() == [1, 0] and d[4].tolist() == [0, 1] and d[8].tolist() == [-1, 0] and d[12].tolist() == [0, -1]
    assert d[2].tolist() == [1, 1] and d[6].tolist() == [-1, 1] and d[10].tolist() == [-1, -1] and d[14].tolist() == [1, -1]
    az = np.degrees(np.arctan2(d[:, 1].astype(np.float64), d[:, 0])) % 360.0
    assert np.allclose(az, 360.0 * np.arange(16) / 16, atol=1e-5)
    assert np.array_equal(d[1], np.array([np.cos(np.pi / 8), np.sin(np.pi / 8)]).astype(np.float32))
    assert directions(1).tolist() == [[1, 0]] and directions(4).tolist() == [[1, 0], [0, 1], [-1, 0], [0, -1]]
    assert np.isfinite(directions(64)).all() and directions(3).shape == (3, 2) and directions(3).any(axis=1).all()
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match=r"directions must lie in \[1, 64\]"):
            directions(bad)
    with pytest.raises(TypeError, match="directions must be an int"):
        directions(2.5)


def test_argument_rules():
    from vulkan_forge_amd._ambient import DEFAULTS, ambient_args, directions
    assert DEFAULTS == {"strength": 0.6, "reach": 64.0, "directions": 16}
    e, s, r, D, d = ambient_args(True, **{"strength": 0.6, "reach": 64.0, "dirs": 16})
    assert (e, s, r, D) == (1, 0.6, 64.0, 16) and np.array_equal(d, directions(16)) and d.flags.c_contiguous
    e, s, r, D, d = ambient_args(False, np.float32(1.0), 1, [(2, 0), (0.5, -3)])
    assert (e, s, r, D) == (0, 1.0, 1.0, 2) and d.dtype == np.float32 and d.tolist() == [[2, 0], [0.5, -3]]     # used as given
    for bad in (1.01, -0.1):
        with pytest.raises(ValueError, match=r"strength must lie in \[0, 1\]"):
            ambient_args(True, bad, 64.0, 16)
    for bad in (0.5, 1024.5):
        with pytest.raises(ValueError, match=r"reach must lie in \[1, 1024\]"):
            ambient_args(True, 0.6, bad, 16)
    for bad in (0, 65):
        with pytest.raises(ValueError, match=r"directions must lie in \[1, 64\]"):
            ambient_args(True, 0.6, 64.0, bad)
    with pytest.raises(ValueError, match=r"directions must lie in \[1, 64\]"):
        ambient_args(True, 0.6, 64.0, np.ones((65, 2), np.float32))
    with pytest.raises(ValueError, match=r"\(D, 2\) array"):
        ambient_args(True, 0.6, 64.0, np.ones((4, 3), np.float32))
    with pytest.raises(ValueError, match="horizontal part"):
        ambient_args(True, 0.6, 64.0, [(1, 0), (0, 0)])
    with pytest.raises(ValueError, match="directions must be finite"):
        ambient_args(True, 0.6, 64.0, [(1, 0), (float("nan"), 1)])
    for k in range(2):
        for bad in (float("nan"), float("inf")):
            a = [0.6, 64.0]
            a[k] = bad
            with pytest.raises(ValueError, match="must be finite"):
                ambient_args(True, *a, 16)
    with pytest.raises(TypeError, match="strength must be a number"):
        ambient_args(True, "dim", 64.0, 16)
    with pytest.raises(TypeError, match="enabled must be a bool"):
        ambient_args("yes", 0.6, 64.0, 16)
