"""Hazed overlay layers without a device: the header, cabi.SYMBOLS and the library agree on the two new entry points,
the header documents them and leaves the haze paragraph's sentence true, NULL handles are refused, the Python methods exist on both
classes of both packages with the documented signatures, and the argument rule refuses what is no bool."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["vf_terrain_set_layer_haze", "vf_terrain_layer_haze"]


def header():
    return open(os.path.join(ROOT, "include", "vf_hip.h")).read()


def test_header_cabi_and_library_agree_on_the_entry_points():
    from vulkan_forge_amd import cabi
    src = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = ctypes.CDLL(cabi.DEFAULT_LIB)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), f"{n} is not declared in include/vf_hip.h"
        assert n in cabi.SYMBOLS and hasattr(lib, n), n
    proto = {n: re.search(n + r"\s*\(([^)]*)\)", src).group(1) for n in NAMES}
    names = {n: [a.split()[-1].lstrip("*") for a in proto[n].split(",")] for n in NAMES}
    assert names["vf_terrain_set_layer_haze"] == ["t", "layer_id", "on"]
    assert names["vf_terrain_layer_haze"] == ["t", "layer_id", "on"]
    assert "int *on" in proto["vf_terrain_layer_haze"] and "int on" in proto["vf_terrain_set_layer_haze"]
    loaded = cabi.load()
    for n in NAMES:
        assert len(getattr(loaded, n).argtypes) == 3, n


def test_the_header_documents_the_calls():
    text = header()
    block = text[text.index("Hazed overlay layers (new"):text.index("int vf_terrain_layer_haze")]
    for n in NAMES:
        assert re.search(r"\* " + n + r":", block), f"{n} has no paragraph in the header's comment"
    for word in ("DESIGN.md 4r", "are not hazed unless their\n * layer asks", "VF_ERR_INVALID", "a polygon\n *   layer cannot take the haze: polygon fills have no depth",
                 "vf_terrain_clear_overlays", "density 0", "byte for byte", "supersampled handles", "both occlude and\n *   take the haze",
                 "does not follow vf_terrain_set_shade_precision"):
        assert word in block, word
    # the haze paragraph stands as it was: overlays are not hazed -- by default
    haze = text[text.index("atmospheric haze: a distance and height fog pass"):]
    assert "are not hazed" in haze and "vf_terrain_set_layer_haze" not in haze


def test_null_handles_are_refused_without_a_device():
    from vulkan_forge_amd import cabi
    lib = cabi.load()
    on = ctypes.c_int(7)
    assert lib.vf_terrain_set_layer_haze(None, 0, 1) == cabi.VF_ERR_INVALID
    assert b"NULL" in lib.vf_last_error()
    assert lib.vf_terrain_layer_haze(None, 0, ctypes.byref(on)) == cabi.VF_ERR_INVALID
    assert b"NULL" in lib.vf_last_error() and on.value == 7


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    import vulkan_forge
    import vulkan_forge_amd
    from vulkan_forge_amd import cabi
    for pkg in (vulkan_forge, vulkan_forge_amd):
        T = getattr(pkg, cls)
        assert re.search(r"set_layer_haze\(self: [\w.]+, layer: (typing\.SupportsInt|int)[^,]*, on: object = True\) -> None", T.set_layer_haze.__doc__), T.set_layer_haze.__doc__
        assert re.search(r"layer_haze\(self: [\w.]+, layer: [^)]*\) -> bool", T.layer_haze.__doc__), T.layer_haze.__doc__
        for name in ("add_points", "add_lines", "add_contours"):
            assert re.search(r"haze: object = False\) -> int", getattr(T, name).__doc__), getattr(T, name).__doc__
        assert "haze" not in T.add_polygons.__doc__
    for name in ("set_layer_haze", "layer_haze"):
        assert callable(getattr(cabi.Terrain, name)), name


def test_argument_rules():
    from vulkan_forge_amd._overlays import haze_arg
    assert haze_arg(True) is True and haze_arg(False) is False and haze_arg(np.bool_(True)) is True
    for bad in (1, 0, "yes", None, 1.0, np.uint8(1), [True]):
        with pytest.raises(TypeError, match="haze must be a bool"):
            haze_arg(bad)
    with pytest.raises(TypeError, match="on must be a bool, got int"):
        haze_arg(1, "on")
