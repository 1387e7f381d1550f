"""The draped image layer without a device: the header, cabi's tables and the library agree on the new entry points and
constants, the Python methods exist on both classes with the documented signatures, and the argument rules refuse what they should."""
import ctypes

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_drape": ["t", "rgba", "iw", "ih", "channels", "extent", "opacity", "filter"],
                "vf_terrain_set_drape_device": ["t", "dev_rgba", "iw", "ih", "extent", "opacity", "filter", "stream"],
                "vf_terrain_clear_drape": ["t"],
                "vf_terrain_drape_info": ["t", "iw", "ih", "extent", "opacity", "filter"],
                "vf_terrain_debug_drape_stage": ["t", "repeats", "ms"]}
CONSTANTS = {"SIZE_MAX": 16384, "NEAREST": 0, "LINEAR": 1}


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import _drape, cabi
    abi.check_entry_points(ENTRY_POINTS)
    abi.check_defines("DRAPE", CONSTANTS.items())
    for k, v in CONSTANTS.items():
        assert getattr(cabi, "VF_DRAPE_" + k) == v, k
    assert (_drape.SIZE_MAX, _drape.NEAREST, _drape.LINEAR) == (16384, 0, 1)
    assert _drape.FILTERS == {"nearest": 0, "linear": 1}


def test_null_arguments_are_refused_without_a_device():
    img = np.zeros((2, 2, 4), np.uint8)
    abi.check_null_refusals([("vf_terrain_set_drape", (img.ctypes.data, 2, 2, 4, None, 1.0, 1)),
                             ("vf_terrain_set_drape_device", (img.ctypes.data, 2, 2, None, 1.0, 1, None)),
                             ("vf_terrain_clear_drape", ()),
                             ("vf_terrain_drape_info", (ctypes.byref(ctypes.c_uint32()), None, None, None, None)),
                             ("vf_terrain_debug_drape_stage", (1, ctypes.byref(ctypes.c_float())))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    A = r"(object|typing\.Any)"
    abi.check_method_docs(cls, {
        "set_drape": rf"set_drape\(self: [\w.]+, image: {A}, \*, extent: {A} = None, opacity: {A} = 1.0, filter: {A} = 'linear'\) -> None",
        "clear_drape": r"clear_drape\(self: [\w.]+\) -> None",
        "drape_info": r"drape_info\(self: [\w.]+\) -> "},
        cabi_methods=("set_drape", "set_drape_device", "clear_drape", "drape_info", "drape_stage"))


def test_argument_rules():
    from vulkan_forge_amd._drape import DEFAULTS, FULL_EXTENT, drape_args, drape_info, drape_params, drape_size
    assert DEFAULTS == {"extent": None, "opacity": 1.0, "filter": "linear"} and FULL_EXTENT == (-1.5, -1.5, 1.5, 1.5)
    rgba = np.arange(2 * 3 * 4, dtype=np.uint8).reshape(2, 3, 4)
    img, iw, ih, ch, ext, op, code = drape_args(rgba)
    assert (iw, ih, ch, op, code) == (3, 2, 4, 1.0, 1) and ext.dtype == np.float32 and ext.tolist() == [-1.5, -1.5, 1.5, 1.5]
    assert img.flags.c_contiguous and np.array_equal(img, rgba)
    img, iw, ih, ch, ext, op, code = drape_args(rgba[:, ::-1, :3], extent=[-1.1, -0.9, 1.3, 1.6], opacity=np.float32(0.5), filter="nearest")
    assert (iw, ih, ch, op, code) == (3, 2, 3, 0.5, 0) and img.flags.c_contiguous and np.array_equal(img, rgba[:, ::-1, :3])
    assert np.array_equal(ext, np.array([-1.1, -0.9, 1.3, 1.6], np.float32))
    assert drape_args(np.zeros((1, 16384, 3), np.uint8))[1:4] == (16384, 1, 3)           # the limit is accepted
    assert drape_args(np.zeros((16384, 1, 4), np.uint8), opacity=0)[1:4] == (1, 16384, 4)
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 5), np.uint8), np.zeros((0, 2, 4), np.uint8),
                np.zeros((2, 0, 4), np.uint8), np.zeros((1, 16385, 3), np.uint8), np.zeros((16385, 1, 3), np.uint8)):
        with pytest.raises(ValueError, match=r"image (must be \(ih, iw, 4\)|width and height must lie in \[1, 16384\])"):
            drape_args(bad)
    for bad in (np.zeros((2, 2, 4), np.float32), np.zeros((2, 2, 4), np.int8), None, "picture.png"):
        with pytest.raises(TypeError, match="image must be"):
            drape_args(bad)
    nan, inf = float("nan"), float("inf")
    for bad in ((0, 0, 0, 1), (0, 0, 1, 0), (1, 0, 0, 1), (0, 1, 1, 0), (0, 0, 1e-46, 1)):
        with pytest.raises(ValueError, match="x1 > x0 and z1 > z0"):
            drape_args(rgba, extent=bad)
    for bad in ((nan, 0, 1, 1), (0, 0, inf, 1), (0, -inf, 1, 1)):
        with pytest.raises(ValueError, match="extent must be finite"):
            drape_args(rgba, extent=bad)
    for bad in ((0, 0, 1), (0, 0, 1, 1, 1), [[0, 0], [1, 1]]):
        with pytest.raises(ValueError, match="extent must be four numbers"):
            drape_args(rgba, extent=bad)
    with pytest.raises(TypeError, match="extent must be four numbers"):
        drape_args(rgba, extent=("a", "b", "c", "d"))
    for bad in (1.01, -0.1):
        with pytest.raises(ValueError, match=r"opacity must lie in \[0, 1\]"):
            drape_args(rgba, opacity=bad)
    for bad in (nan, inf):
        with pytest.raises(ValueError, match="opacity must be finite"):
            drape_args(rgba, opacity=bad)
    with pytest.raises(TypeError, match="opacity must be a number"):
        drape_args(rgba, opacity="half")
    with pytest.raises(ValueError, match="filter must be 'linear' or 'nearest'"):
        drape_args(rgba, filter="cubic")
    with pytest.raises(TypeError, match="filter must be 'linear' or 'nearest'"):
        drape_args(rgba, filter=1)
    assert drape_params(None, 1, "linear")[1:] == (1.0, 1)
    assert drape_size(16384, 1) == (16384, 1)
    for bad in ((0, 1), (1, 0), (16385, 1)):
        with pytest.raises(ValueError, match=r"\[1, 16384\]"):
            drape_size(*bad)
    with pytest.raises(TypeError, match="must be an int"):
        drape_size(2.5, 1)
    assert drape_info(0, 0, (0, 0, 0, 0), 0.0, 0) is None
    assert drape_info(37, 53, (-1.5, -1.5, 1.5, 1.5), 0.5, 0) == {"width": 37, "height": 53, "extent": (-1.5, -1.5, 1.5, 1.5), "opacity": 0.5, "filter": "nearest"}
