"""The call shapes the two binding layers repeat (the helpers of host/module.cpp and cabi.py), pinned from outside on
both classes of the extension and on cabi.Terrain: the eight per-vertex field getters return the same bits through either layer and
through the *_field_device calls, and read a resting field from its cache; a getter refused by the library raises the library's text
and leaves the object usable; every setter and clear_* makes the next frame-plane getter draw again, clear_overlays does not; an
occluding point layer refused on a supersampled object was never made.  Frame 64 x 48, grid 17: one block of the scans, one tile of
the fills -- the kernels have their own tests; what varies here is the route to them."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
from overlay_scenes import CAMERAS, heights
from support import bits

W, H, GRID = 64, 48, 17
SHADOWS = dict(strength=0.8, softness=0.05, bias=0.01)
AMBIENT = dict(strength=0.6, reach=8.0, directions=4)
SCAN = dict(eye_height=0.1, target_height=0.02, softness=0.05, bias=0.01)
OBSERVER = (0.41, -0.87)
OBSERVERS = [(-1.5, -1.5), (0.0, 0.0), (0.9, 1.2)]
SUNS = np.array([(0.9, 0.3, 0.31), (-0.3, 0.25, 0.9)], np.float32)
EXPOSURE = dict(incidence=True, softness=0.05, bias=0.01)
LEVEL = 0.0
HAZE = dict(start=0.5, falloff=0.8, max_opacity=0.9)

# field -> (getter of both layers, scan counter of the extension, of cabi.Terrain, the *_field_device call or None)
FIELDS = {
    "shadow_field": ("debug_shadow_scans", "shadow_scans", "shadow_field_device"),
    "sky_view_field": ("debug_ambient_scans", "ambient_scans", "sky_view_field_device"),
    "viewshed_field": ("debug_viewshed_scans", "viewshed_scans", "viewshed_field_device"),
    "cumulative_viewshed_field": ("debug_cumulative_viewshed_scans", "cumulative_viewshed_scans", "cumulative_viewshed_field_device"),
    "sun_exposure_field": ("debug_sun_exposure_scans", "sun_exposure_scans", "sun_exposure_field_device"),
    "flood_field": ("debug_flood_scans", "flood_scans", "flood_field_device"),
    "spill_field": ("debug_spill_scans", "spill_scans", "spill_field_device"),
    "sink_depth_field": ("debug_spill_scans", "spill_scans", None),     # (the spill's second plane: its counter)
}
# the getters that need something set first, and what the library says before that
UNSET = {
    "viewshed_field": "no observer set (vf_terrain_set_viewshed)",
    "cumulative_viewshed_field": "no observers set (vf_terrain_set_cumulative_viewshed)",
    "sun_exposure_field": "no suns set (vf_terrain_set_sun_exposure)",
    "flood_field": "no flood set (vf_terrain_set_flood)",
    "spill_field": "no spill set (vf_terrain_set_spill)",
}


def set_analyses(x):
    """the seven analyses and the haze, with the same parameters on whichever surface `x` is"""
    x.set_shadows(True, **SHADOWS)
    x.set_ambient_occlusion(True, **AMBIENT)
    x.set_viewshed(OBSERVER, **SCAN)
    x.set_cumulative_viewshed(OBSERVERS, **SCAN)
    x.set_sun_exposure(SUNS, **EXPOSURE)
    x.set_flood(LEVEL, "edges")
    x.set_spill("edges")
    x.set_haze(0.5, **HAZE)


def surfaces(cls, analyses=True):
    """an object of the extension's class `cls` and a cabi.Terrain in the same state: the object's uniforms and, for the Scene, the
    same heights (a TerrainSpike has no height setter: both stand on the library's flat default)"""
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    obj = getattr(vf, cls)(W, H, grid=GRID)
    twin = cabi.Terrain(W, H, GRID, vf.colormap_rgba8("viridis"))
    if cls == "Scene":
        obj.set_height_from_r32f(heights())
        twin.set_height(heights())
    twin.set_uniforms(obj.debug_uniforms_f32())
    if analyses:
        set_analyses(obj)
        set_analyses(twin)
    return obj, twin


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_the_field_getters_return_the_same_bits_through_both_layers_and_scan_once(cls):
    obj, twin = surfaces(cls)
    for name, (ext_scans, abi_scans, _) in FIELDS.items():
        got, want = getattr(obj, name)(), getattr(twin, name)()
        assert got.shape == want.shape == (GRID, GRID) and got.dtype == want.dtype == np.float32, name
        assert np.array_equal(bits(got), bits(want)), name
        assert np.array_equal(bits(getattr(obj, name)()), bits(got)) and np.array_equal(bits(getattr(twin, name)()), bits(want)), name
        assert (getattr(obj, ext_scans)(), getattr(twin, abi_scans)()) == (1, 1), name
        if cls == "Scene":                                    # (a comparison of constants would not tell one getter from another)
            assert (got != got.flat[0]).any(), f"the {name} is constant"
    got = obj.haze_opacity()                                  # (draws the frame first)
    twin.render()
    want = twin.haze_opacity()
    assert got.shape == want.shape == (H, W) and np.array_equal(bits(got), bits(want))
    assert (got > 0).any() and (got == 0).any()
    for name, (ext_scans, abi_scans, _) in FIELDS.items():    # the frames read the same caches
        assert (getattr(obj, ext_scans)(), getattr(twin, abi_scans)()) == (1, 1), name
    twin.close()


def torch_check():
    """(a process of its own: torch is imported before the library, one HIP runtime per process)"""
    import torch
    obj, twin = surfaces("Scene")
    stream = torch.cuda.Stream()
    for name, (_, abi_scans, device) in FIELDS.items():
        if device is None:
            continue
        want = getattr(obj, name)()
        dst = torch.full((GRID, GRID), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        getattr(twin, device)(dst.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(bits(dst.cpu().numpy()), bits(want)), name
        assert np.array_equal(bits(getattr(twin, name)()), bits(want)), name
        assert getattr(twin, abi_scans)() == 1, name
    twin.close()
    print("BINDING SURFACES TORCH OK")


def test_the_field_device_calls_return_those_bits_in_torch_tensors():
    support.run_check(os.path.basename(__file__), "BINDING SURFACES TORCH OK")


@pytest.mark.parametrize("cls", ["Scene", "TerrainSpike"])
def test_a_refused_getter_raises_the_librarys_text_and_leaves_the_object_usable(cls):
    from vulkan_forge_amd import cabi
    obj, twin = surfaces(cls, analyses=False)
    for name, text in UNSET.items():
        with pytest.raises(RuntimeError, match=re.escape(text)) as e:
            getattr(obj, name)()
        assert type(e.value) is RuntimeError and str(e.value) == text, name
        obj.debug_uniforms_f32()                              # (raises while the object is borrowed)
        with pytest.raises(cabi.VfError) as e:
            getattr(twin, name)()
        assert str(e.value) == text, name
    # the borrow went back and the GIL was taken again on the error path: every other call works
    assert np.array_equal(bits(obj.shadow_field()), bits(twin.shadow_field())) and obj.debug_shadow_scans() == 1
    set_analyses(obj)
    set_analyses(twin)
    for name in UNSET:
        assert np.array_equal(bits(getattr(obj, name)()), bits(getattr(twin, name)())), name
    assert obj.render_rgba().shape == (H, W, 4)
    twin.close()


def draws(obj):
    """does the next render_depth() draw a frame?  (the timing window starts empty: last_timings() refuses until a frame is drawn)"""
    obj.enable_timing(True)
    obj.render_depth()
    try:
        return obj.last_timings()["frames"]
    except RuntimeError as e:
        assert str(e) == "timing not enabled or nothing rendered"
        return 0


def test_every_setter_and_clear_makes_the_next_frame_getter_draw_and_clear_overlays_does_not():
    import vulkan_forge_amd as vf
    s = vf.Scene(W, H, grid=GRID)
    image = np.random.default_rng(5).integers(0, 256, (8, 12, 4), dtype=np.uint8)
    assert draws(s) == 1 and draws(s) == 0                    # a resting object draws once
    steps = [
        ("set_height_from_r32f", lambda: s.set_height_from_r32f(heights())),
        ("set_camera_look_at", lambda: s.set_camera_look_at(*CAMERAS["fill"])),
        ("set_sun", lambda: s.set_sun(30.0, 120.0)),
        ("set_exposure", lambda: s.set_exposure(1.5)),
        ("set_shadows", lambda: s.set_shadows(True, **SHADOWS)),
        ("set_ambient_occlusion", lambda: s.set_ambient_occlusion(True, **AMBIENT)),
        ("set_drape", lambda: s.set_drape(image, opacity=0.7)),
        ("set_drape_mipmaps", lambda: s.set_drape_mipmaps(True, bias=0.5)),
        ("set_drape_anisotropy", lambda: s.set_drape_anisotropy(4)),
        ("clear_drape", s.clear_drape),
        ("set_viewshed", lambda: s.set_viewshed(OBSERVER, **SCAN)),
        ("clear_viewshed", s.clear_viewshed),
        ("set_cumulative_viewshed", lambda: s.set_cumulative_viewshed(OBSERVERS, **SCAN)),
        ("clear_cumulative_viewshed", s.clear_cumulative_viewshed),
        ("set_sun_exposure", lambda: s.set_sun_exposure(SUNS, **EXPOSURE)),
        ("clear_sun_exposure", s.clear_sun_exposure),
        ("set_haze", lambda: s.set_haze(0.5, **HAZE)),
        ("clear_haze", s.clear_haze),
        ("set_flood", lambda: s.set_flood(LEVEL, "edges")),
        ("clear_flood", s.clear_flood),
        ("set_spill", lambda: s.set_spill("edges")),
        ("clear_spill", s.clear_spill),
    ]
    for name, call in steps:
        call()
        assert draws(s) == 1, f"{name} did not make render_depth() draw"
        assert draws(s) == 0, f"the frame after {name} was drawn twice"
    # haze_opacity() takes the frame render_depth() left, and draws after a setter too
    assert s.haze_opacity().shape == (H, W) and draws(s) == 0
    s.set_exposure(1.0)
    s.enable_timing(True)
    s.haze_opacity()
    assert s.last_timings()["frames"] == 1 and draws(s) == 0
    # overlays are composited behind the planes: neither a new layer nor clear_overlays() draws the terrain again
    layer = s.add_points([(0.0, 0.2, 0.0)], size_px=6.0, haze=True)
    assert s.layer_primitive_count(layer) == 1 and s.layer_haze(layer) and draws(s) == 0
    s.clear_overlays()
    assert draws(s) == 0
    with pytest.raises(RuntimeError, match="no overlay layer with that id"):
        s.layer_primitive_count(layer)


def test_an_occluding_layer_refused_on_a_supersampled_object_was_never_made():
    import vulkan_forge_amd as vf
    s = vf.Scene(W, H, grid=GRID, supersample=2)
    s.set_height_from_r32f(heights())
    refusal = "the handle is supersampled: occluding overlay layers are not supported"
    with pytest.raises(RuntimeError, match=refusal):
        s.add_points([(0.0, 0.2, 0.0)], occlude=True)
    with pytest.raises(RuntimeError, match=refusal):
        s.add_lines([[(0.0, 0.2, 0.0), (0.5, 0.2, 0.5)]], occlude=True)
    with pytest.raises(RuntimeError, match=refusal):
        s.add_contours([0.0], occlude=True)
    with pytest.raises(RuntimeError, match="no overlay layer with that id"):
        s.layer_primitive_count(0)                            # (the id the first layer gets, below)
    layer = s.add_points([(0.0, 0.2, 0.0)], haze=True)
    assert layer == 0 and s.layer_primitive_count(0) == 1 and s.layer_haze(0)
    assert s.render_rgba().shape == (H, W, 4)
    # render_samples(), the third frame-plane getter, draws after a setter and not on a resting object
    s.set_exposure(1.5)
    s.enable_timing(True)
    assert s.render_samples().shape == (2 * H, 2 * W, 4) and s.last_timings()["frames"] == 1
    assert draws(s) == 0 and s.render_depth().shape == (2 * H, 2 * W)


if __name__ == "__main__":
    torch_check()
