"""Hazed overlay layers without a device: the header, cabi.SYMBOLS and the library agree on the two new entry points,
the header documents them and leaves the haze paragraph's sentence true, NULL handles are refused, the Python methods exist on both
classes of both packages with the documented signatures, and the argument rule refuses what is no bool."""
import ctypes
import re

import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_set_layer_haze": ["t", "layer_id", "on"], "vf_terrain_layer_haze": ["t", "layer_id", "on"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    abi.check_entry_points(ENTRY_POINTS)
    src = abi.code()
    proto = {n: re.search(n + r"\s*\(([^)]*)\)", src).group(1) for n in ENTRY_POINTS}
    assert "int *on" in proto["vf_terrain_layer_haze"] and "int on" in proto["vf_terrain_set_layer_haze"]


def test_the_header_documents_the_calls():
    abi.check_header_documents("Hazed overlay layers (new", list(ENTRY_POINTS),
                               ("DESIGN.md 4r", "are not hazed unless their\n * layer asks", "VF_ERR_INVALID",
                                "a polygon\n *   layer cannot take the haze: polygon fills have no depth",
                                "vf_terrain_clear_overlays", "density 0", "byte for byte", "supersampled handles", "both occlude and\n *   take the haze",
                                "does not follow vf_terrain_set_shade_precision"), until="int vf_terrain_layer_haze")
    # the haze paragraph stands as it was: overlays are not hazed -- by default
    text = abi.header_text()
    haze = text[text.index("atmospheric haze: a distance and height fog pass"):]
    assert "are not hazed" in haze and "vf_terrain_set_layer_haze" not in haze


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    lib = cabi.load()
    on = ctypes.c_int(7)
    abi.check_null_refusals([("vf_terrain_set_layer_haze", (0, 1))])
    assert b"NULL" in lib.vf_last_error()
    abi.check_null_refusals([("vf_terrain_layer_haze", (0, ctypes.byref(on)))])
    assert b"NULL" in lib.vf_last_error() and on.value == 7


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "set_layer_haze": r"set_layer_haze\(self: [\w.]+, layer: (typing\.SupportsInt|int)[^,]*, on: object = True\) -> None",
        "layer_haze": r"layer_haze\(self: [\w.]+, layer: [^)]*\) -> bool",
        "add_points": r"haze: object = False\) -> int", "add_lines": r"haze: object = False\) -> int", "add_contours": r"haze: object = False\) -> int",
        "add_polygons": r"\A(?!(.|\n)*haze)"},
        cabi_methods=("set_layer_haze", "layer_haze"))


def test_argument_rules():
    from vulkan_forge_amd._overlays import haze_arg
    assert haze_arg(True) is True and haze_arg(False) is False and haze_arg(np.bool_(True)) is True
    for bad in (1, 0, "yes", None, 1.0, np.uint8(1), [True]):
        with pytest.raises(TypeError, match="haze must be a bool"):
            haze_arg(bad)
    with pytest.raises(TypeError, match="on must be a bool, got int"):
        haze_arg(1, "on")
