"""Supersampled frames without a device: the header, cabi.SYMBOLS and the library agree on the five entry points and
the constant, the ctypes prototypes have the header's argument counts, NULL handles are refused, and the Python argument rules raise
ValueError before the library is called."""
import ctypes
import re

import numpy as np
import pytest

import abi_support as abi

ARGS = {
    "vf_terrain_create_supersampled": ["ctx", "width", "height", "grid", "lut_rgba8", "lut_is_srgb", "factor", "out"],
    "vf_terrain_supersampling": ["t", "factor", "sample_width", "sample_height"],
    "vf_terrain_read_samples": ["t", "dst"],
    "vf_terrain_samples_device": ["t", "dev_dst", "stream"],
    "vf_terrain_debug_resolve_stage": ["t", "repeats", "ms"],
}


def test_header_cabi_and_library_agree_on_the_entry_points():
    abi.check_entry_points(ARGS)
    assert re.search(r"vf_terrain_create_supersampled\s*\([^)]*\blut_rgba8\[1024\],", abi.code())
    abi.prototypes(["vf_terrain_create"])                                      # (stays, and means factor 1)


def test_the_constant():
    from vulkan_forge_amd import _supersample, cabi
    m = re.search(r"#define\s+VF_SUPERSAMPLE_MAX\s+(\d+)", abi.code())
    assert m and int(m.group(1)) == 4 == cabi.VF_SUPERSAMPLE_MAX == _supersample.SUPERSAMPLE_MAX


def test_null_handles_are_refused_without_a_device():
    out = np.zeros(16, np.uint8)
    lut = np.zeros(1024, np.uint8)
    abi.check_null_refusals([("vf_terrain_create_supersampled", (8, 8, 8, lut.ctypes.data, 1, 2, ctypes.byref(ctypes.c_void_p()))),
                             ("vf_terrain_supersampling", (ctypes.byref(ctypes.c_uint32()), None, None)),
                             ("vf_terrain_read_samples", (out.ctypes.data,)),
                             ("vf_terrain_samples_device", (None, None)),
                             ("vf_terrain_debug_resolve_stage", (1, ctypes.byref(ctypes.c_float())))])


def test_the_argument_rules():
    from vulkan_forge_amd._supersample import representative, sample_size, supersample_args
    assert [supersample_args(64, 48, f) for f in (1, 2, 3, 4)] == [1, 2, 3, 4]
    assert supersample_args(16384, 16384, 1) == 1 and supersample_args(8192, 8192, 2) == 2 and supersample_args(4096, 4096, 4) == 4
    assert supersample_args(64, 48, np.int64(3)) == 3
    for bad in (0, 5, -1, 16):
        with pytest.raises(ValueError, match=r"supersample must be in 1\.\.4"):
            supersample_args(64, 48, bad)
    with pytest.raises(ValueError, match=r"needs 16388 x 32 samples"):
        supersample_args(4097, 8, 4)
    with pytest.raises(ValueError, match=r"needs 24 x 16386 samples"):
        supersample_args(8, 5462, 3)
    for bad in (2.0, "2", None, True):
        with pytest.raises(TypeError, match="supersample must be an integer"):
            supersample_args(64, 48, bad)
    assert sample_size(71, 45, 3) == (213, 135)
    assert representative(5, 7, 1) == (5, 7) and representative(5, 7, 2) == (11, 15) and representative(5, 7, 3) == (16, 22) and representative(0, 0, 4) == (2, 2)


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_the_classes_raise_value_errors_before_the_library_is_called(cls):
    import vulkan_forge
    import vulkan_forge_amd
    for pkg in (vulkan_forge, vulkan_forge_amd):
        T = getattr(pkg, cls)
        assert "supersample: object = 1" in T.__init__.__doc__, T.__init__.__doc__
        for name in ("supersample", "samples", "sample_size"):
            assert isinstance(getattr(T, name), property), name
        assert re.search(r"render_samples\(self: [\w.]+\) -> numpy", T.render_samples.__doc__), T.render_samples.__doc__
        for bad in (0, 5):
            with pytest.raises(ValueError, match=r"supersample must be in 1\.\.4"):
                T(64, 48, supersample=bad)
        with pytest.raises(ValueError, match="16388 x 32 samples"):
            T(4097, 8, supersample=4)
        with pytest.raises(ValueError, match="24 x 16386 samples"):
            T(8, 5462, grid=8, supersample=3)
        with pytest.raises(TypeError):
            T(64, 48, 32, "viridis", 2)                               # keyword only
