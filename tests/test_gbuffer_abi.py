"""Geometry buffers without a device: the header, cabi.SYMBOLS and the library agree on the new entry points, the
Python methods exist on both classes with the documented signatures, and the argument rules refuse what they should."""
import numpy as np
import pytest

import abi_support as abi

ENTRY_POINTS = {"vf_terrain_gbuffer_device": ["t", "dev_depth", "dev_position", "dev_normal", "dev_primitive", "stream"],
                "vf_terrain_read_gbuffer": ["t", "depth", "position", "normal", "primitive"],
                "vf_terrain_pick": ["t", "pixels_xy", "n", "out8"],
                "vf_terrain_debug_gbuffer_stage": ["t", "planes", "repeats", "ms"]}


def test_header_cabi_and_library_agree_on_the_entry_points():
    abi.check_entry_points(ENTRY_POINTS)


def test_null_handles_are_refused_without_a_device():
    out = np.zeros(8, np.float32)
    abi.check_null_refusals([("vf_terrain_read_gbuffer", (out.ctypes.data, None, None, None)),
                             ("vf_terrain_gbuffer_device", (None, None, None, None, None)),
                             ("vf_terrain_pick", (None, 0, None))])


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_methods_exist_on_both_classes(cls):
    abi.check_method_docs(cls, {
        "render_gbuffer": r"planes: object = \('depth', 'position', 'normal', 'primitive'\)(.|\n)*-> dict",
        "render_depth": r"render_depth\(self: [\w.]+\) -> numpy",
        "pick": r"pick\(self: [\w.]+, pixels: object\) -> dict"})


def test_plane_rules():
    from vulkan_forge_amd._gbuffer import PLANES, plane_args
    assert list(PLANES) == ["depth", "position", "normal", "primitive"]
    assert plane_args(["normal", "depth"]) == ("normal", "depth")
    assert plane_args(k for k in PLANES) == tuple(PLANES)
    with pytest.raises(ValueError, match="unknown plane 'colour'"):
        plane_args(("depth", "colour"))
    with pytest.raises(ValueError, match="'depth' more than once"):
        plane_args(("depth", "normal", "depth"))
    with pytest.raises(ValueError, match="at least one"):
        plane_args(())
    with pytest.raises(TypeError, match="the string 'depth'"):
        plane_args("depth")
    with pytest.raises(TypeError, match="sequence of plane names"):
        plane_args(None)
    with pytest.raises(TypeError, match="must be strings"):
        plane_args(("depth", 1))


def test_pixel_rules():
    from vulkan_forge_amd._gbuffer import pick_result, pixel_args
    px = pixel_args(np.array([[3, 2], [0, 0], [9, 4]], np.int64), 10, 5)
    assert px.dtype == np.int32 and px.flags.c_contiguous and px.tolist() == [[3, 2], [0, 0], [9, 4]]
    assert pixel_args(np.array([[1, 2]], np.uint8)[:, ::-1], 10, 5).tolist() == [[2, 1]]
    assert pixel_args(np.zeros((0, 2), np.int32), 10, 5).shape == (0, 2)
    with pytest.raises(TypeError, match="integer array, got dtype float64"):
        pixel_args(np.zeros((3, 2)), 10, 5)
    with pytest.raises(TypeError, match="integer array, got dtype bool"):
        pixel_args(np.zeros((3, 2), bool), 10, 5)
    with pytest.raises(ValueError, match=r"shape \(N, 2\)"):
        pixel_args(np.zeros((3, 3), np.int32), 10, 5)
    with pytest.raises(ValueError, match=r"shape \(N, 2\)"):
        pixel_args(np.zeros(4, np.int32), 10, 5)
    for bad in ([10, 0], [0, 5], [-1, 0], [0, -1]):
        with pytest.raises(ValueError, match=r"pixel 1 \(-?\d+, -?\d+\) lies outside the 10 x 5 frame"):
            pixel_args([[0, 0], bad], 10, 5)
    words = np.arange(16, dtype=np.uint32).reshape(2, 8)
    r = pick_result(words)
    assert r["depth"].shape == (2,) and r["position"].shape == (2, 3) and r["normal"].shape == (2, 3)
    assert r["primitive"].dtype == np.uint32 and r["primitive"].tolist() == [7, 15]
    assert r["position"].view(np.uint32).tolist() == [[1, 2, 3], [9, 10, 11]]
