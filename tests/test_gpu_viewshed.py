"""Viewshed analysis on the GPU equals the CPU model (tests/viewshed_model) bit for bit: the field for observers on
the corners, the edges, inside and outside the grid, on grids that need carries, are no multiple of 64 and are long, through both
entry points; the tinted frame over three cameras, two sizes, both shade modes and both precisions, with and without a radius and
with either tint alone; over shadows, ambient occlusion and a drape; under overlays; and nothing else moves -- the frame with the
viewshed off or cleared, geometry buffers, visibility, the scan counter of a resting scene, the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import viewshed_model as vsm
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from support import assert_field, assert_frame, bits, terrain, uniforms, vf, viridis  # noqa: F401
from viewshed_model import SCENE_OBSERVER, SCENE_PARAMS

# (x, z) in world units at spacing 1: the four corners, two edge midpoints, the centre, an off-centre vertex, outside the grid (clamped)
OBSERVERS = [(-1.5, -1.5), (1.5, -1.5), (-1.5, 1.5), (1.5, 1.5), (0.0, -1.5), (1.5, 0.1), (0.0, 0.0), (0.41, -0.87), (7.0, -0.3)]
PARAMS = dict(eye_height=0.4, target_height=0.02, softness=0.05, bias=0.01)
RED, GREEN = (255, 0, 0, 128), (64, 255, 96, 96)


@pytest.mark.parametrize("grid,observers", [(130, OBSERVERS), (203, OBSERVERS), (257, OBSERVERS), (1025, OBSERVERS[7:8])])
def test_field_equals_the_model(grid, observers):
    h = heights(4, (97, 131))
    t = terrain(64, 64, grid, h)
    u = uniforms(64, 64, exag=0.6)
    t.set_uniforms(u)
    hidden = 0
    for obs in observers:
        t.set_viewshed(obs, enabled=False, **PARAMS)          # the field does not need the viewshed enabled for drawing
        got = t.viewshed_field()
        want, v = vsm.field(u, h, grid, obs, **PARAMS)
        assert got.shape == (grid, grid) and got.dtype == np.float32
        assert_field(got, want, f"grid {grid} observer {obs} -> vertex {v}")
        info = t.viewshed_info()
        assert info["vertex"] == v and info["enabled"] is False and got[v[1], v[0]] == 1.0
        hidden += int((want < 1).sum())
    assert hidden > len(observers) * grid * grid // 10         # (the comparison is not one of open ground)
    assert vsm.observer_vertex(OBSERVERS[-1], 1.0, grid)[0] == grid - 1
    t.close()


def test_field_into_device_memory_on_a_stream_of_the_callers():
    support.run_check("viewshed_torch_check.py", "VIEWSHED TORCH OK")


# both tints; the hidden tint alone, inside a radius; the visible tint alone; both inside a larger radius
TINTS = [dict(visible_rgba=GREEN, hidden_rgba=RED), dict(visible_rgba=(64, 255, 96, 0), hidden_rgba=RED, radius=0.8),
         dict(visible_rgba=GREEN, hidden_rgba=(0, 0, 0, 0)), dict(visible_rgba=GREEN, hidden_rgba=RED, radius=1.0)]


@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("size", [(640, 360), (257, 131)])
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, size, mode):
    W, H = size
    h = heights()
    seen = None
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        plain = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
        if seen is None:
            rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
            seen, v = vsm.field(u, h, GRID, SCENE_OBSERVER, **SCENE_PARAMS)
            assert np.array_equal(plain, rgba.reshape(H, W, 4))                # (the exact frame is the oracle's)
        covered = vis != 0
        for tint in TINTS:
            s.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, **tint)
            got = s.render_rgba()
            # the tint blends over the frame's own bytes: the oracle's in exact precision, the fast frame's in fast
            want, sv = vsm.frame(plain, vis, u, h, GRID, seen, v, **tint)
            assert_frame(got, want, f"{precision} {cam} {size} {mode} {tint}")
            treated = sv >= 0
            if "radius" not in tint:
                frac = float((sv[covered] < 0.5).mean())
                assert np.array_equal(treated, covered) and 0.1 < frac < 0.9, frac
            elif cam != "near":
                assert treated.any() and (covered & ~treated).any()
            assert (got != plain).any() and np.array_equal(got[~treated], plain[~treated])
            assert np.array_equal(s.render_rgba(), got)
        assert_field(s.viewshed_field(), seen, "the scene's field")
        assert s.debug_viewshed_scans() == 1                                     # colours and radius: no new field


def test_the_tint_lies_over_shadows_ambient_occlusion_and_a_drape(vf):
    from shadow_model import SCENE_PARAMS as SHADOW_PARAMS, SCENE_SUN_DEG
    W, H = 640, 360
    h = heights()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 50, 4), dtype=np.uint8)
    frames = {}
    for tinted in (False, True):
        s = scene(vf, W, H, h, "default", "exact")
        s.set_sun(*SCENE_SUN_DEG)
        s.set_shadows(True, **SHADOW_PARAMS)
        s.set_ambient_occlusion(True)
        s.set_drape(img, extent=(-1.0, -1.2, 0.9, 1.1), opacity=0.8)
        if tinted:
            s.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, visible_rgba=GREEN, hidden_rgba=RED, radius=1.5)
        frames[tinted] = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
    _, vis = support.oracle_frame(u, W, H, GRID, h)
    seen, v = vsm.field(u, h, GRID, SCENE_OBSERVER, **SCENE_PARAMS)
    want, sv = vsm.frame(frames[False], vis, u, h, GRID, seen, v, visible_rgba=GREEN, hidden_rgba=RED, radius=1.5)
    plain = scene(vf, W, H, h, "default", "exact").render_rgba()
    assert (frames[False] != plain).any() and (want != frames[False]).any()
    assert_frame(frames[True], want, "tint over shadows, ambient occlusion and a drape")


def test_overlays_composite_over_the_tinted_frame(vf):
    import occlusion_model as ocm
    W, H = 640, 360
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    s.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, visible_rgba=GREEN, hidden_rgba=RED)
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 1500
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.08, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(80)]
    poly = [np.array([[-0.6, 0.05, -0.6], [0.7, 0.05, -0.5], [0.1, 0.05, 0.8]], np.float32)]
    info = s.viewshed_info()
    marker = np.array([info["observer_xyz"]], np.float32)                          # the observer's own vertex, in the overlays' frame
    calls = [("add_points", (pts,), dict(size_px=5.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)),
             ("add_lines", (paths,), dict(width_px=3.0, rgba=(0, 255, 0, 200), drape=True)),
             ("add_polygons", (poly,), dict(fill_rgba=(0, 90, 255, 160))),
             ("add_points", (marker,), dict(size_px=9.0, rgba=(255, 255, 0, 255)))]
    L = apply(vf, s, calls, ocm.Layers())
    rgba, vis = support.oracle_frame(u, W, H, GRID, h)
    seen, v = vsm.field(u, h, GRID, SCENE_OBSERVER, **SCENE_PARAMS)
    assert info["vertex"] == v and info["enabled"] is True and info["eye_y"] == pytest.approx(info["observer_xyz"][1] + SCENE_PARAMS["eye_height"])
    base, _ = vsm.frame(rgba, vis, u, h, GRID, seen, v, visible_rgba=GREEN, hidden_rgba=RED)
    want = ocm.composite(base, vis, u, h, GRID, L)
    got = s.render_rgba()
    assert (base != rgba.reshape(H, W, 4)).any() and (want != base).any()
    assert not np.array_equal(want, ocm.pm.composite(base, u, h, GRID, L))         # (the occluding layer matters)
    assert_frame(got, want, "overlays over the tint")


def test_the_frame_the_gbuffers_and_the_visibility_are_unchanged_when_off(vf):
    W, H = 640, 360
    h = heights(5)
    never = scene(vf, W, H, h)
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    visib = never.debug_visibility().copy()
    s = scene(vf, W, H, h)
    assert s.viewshed_info()["enabled"] is False and s.viewshed_info()["vertex"] is None
    assert np.array_equal(s.render_rgba(), want)              # before enabling
    s.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, hidden_rgba=RED)
    tinted = s.render_rgba().copy()
    assert (tinted != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    assert np.array_equal(s.render_rgba(), tinted)
    s.set_viewshed(SCENE_OBSERVER, enabled=False, **SCENE_PARAMS, hidden_rgba=RED)
    assert np.array_equal(s.render_rgba(), want)              # off: the field is still there to be read
    assert s.viewshed_field().shape == (GRID, GRID) and s.viewshed_info()["vertex"] is not None
    s.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, hidden_rgba=RED)
    assert np.array_equal(s.render_rgba(), tinted)
    s.clear_viewshed()
    assert np.array_equal(s.render_rgba(), want)              # cleared
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert s.viewshed_info()["vertex"] is None
    with pytest.raises(RuntimeError, match="no observer set"):
        s.viewshed_field()
    sp = vf.TerrainSpike(160, 120, grid=48)
    sp.set_viewshed((0.2, 0.3))
    assert sp.viewshed_field().shape == (48, 48)
    assert sp.render_rgba().shape == (120, 160, 4)


def test_the_field_follows_its_inputs_and_rests_otherwise(vf):
    W, H = 320, 200
    lut = viridis()
    h = heights(3)
    t = terrain(W, H, GRID, h, lut)
    t.set_shade_precision(0)
    tint = dict(visible_rgba=GREEN, hidden_rgba=RED)
    t.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, **tint)

    def check(u, hh, obs, what, params=SCENE_PARAMS, **kw):
        import oracle
        t.render()
        got = t.read_rgba()
        rgba, vis = oracle.render_terrain(u, W, H, GRID, hh, lut, want_vis=True, nthreads=8)
        seen, v = vsm.field(u, hh, GRID, obs, **params)
        want, sv = vsm.frame(rgba, vis, u, hh, GRID, seen, v, **{**tint, **kw})
        assert (want != rgba.reshape(H, W, 4)).any(), what
        assert_frame(got.reshape(H, W, 4), want, what)

    u = uniforms(W, H)
    t.set_uniforms(u)
    assert t.viewshed_scans() == 0
    check(u, h, SCENE_OBSERVER, "first frame")
    assert t.viewshed_scans() == 1
    for _ in range(3):                                        # a resting scene pays once
        t.render()
    t.read_rgba()
    assert t.viewshed_scans() == 1
    # what the field does not depend on: colours, radius, camera, sun, a spacing that leaves the observer's vertex where it was
    tint = dict(visible_rgba=(0, 0, 255, 200), hidden_rgba=(20, 20, 20, 90))
    t.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, **tint, radius=0.9)
    check(u, h, SCENE_OBSERVER, "new colours and a radius", radius=0.9)
    t.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, **tint)
    u = uniforms(W, H, cam="fill", sun=(0.3, 0.8, -0.5))
    t.set_uniforms(u)
    check(u, h, SCENE_OBSERVER, "new camera and sun")
    assert t.viewshed_scans() == 1
    step = 3.0 / (GRID - 1)
    nudged = (SCENE_OBSERVER[0] + 0.2 * step, SCENE_OBSERVER[1] - 0.2 * step)
    assert vsm.observer_vertex(nudged, 1.0, GRID) == vsm.observer_vertex(SCENE_OBSERVER, 1.0, GRID)
    t.set_viewshed(nudged, **SCENE_PARAMS, **tint)
    t.render()
    assert t.viewshed_scans() == 1                            # (an observer that moves inside its vertex's cell)
    t.set_viewshed((0.0, 0.0), **SCENE_PARAMS, **tint)
    t.render()
    assert t.viewshed_scans() == 2                            # (the centre is another vertex ...)
    u = uniforms(W, H, cam="fill", sun=(0.3, 0.8, -0.5), spacing=1.7)
    t.set_uniforms(u)
    t.render()
    assert t.viewshed_scans() == 2                            # (... which stays the centre at any spacing)
    # what it does depend on
    t.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, **tint)
    u = uniforms(W, H)
    t.set_uniforms(u)
    check(u, h, SCENE_OBSERVER, "back to the first observer")
    assert t.viewshed_scans() == 3
    u = uniforms(W, H, exag=1.6)
    t.set_uniforms(u)
    check(u, h, SCENE_OBSERVER, "new exaggeration")
    assert t.viewshed_scans() == 4
    h2 = heights(9)
    t.set_height(h2)
    check(u, h2, SCENE_OBSERVER, "new heights")                # (the setting survives a height upload)
    assert t.viewshed_scans() == 5
    params = dict(SCENE_PARAMS)
    for k, (name, value) in enumerate((("eye_height", 1.4), ("target_height", 0.05), ("softness", 0.2), ("bias", 0.02))):
        params[name] = value
        t.set_viewshed(SCENE_OBSERVER, **params, **tint)
        check(u, h2, SCENE_OBSERVER, f"new {name}", params=params)
        assert t.viewshed_scans() == 6 + k
    before = t.viewshed_scans()
    ms = t.viewshed_stage(3)
    assert ms[0] > 0 and ms[1] > 0 and t.viewshed_scans() == before   # (diagnostic launches are not the handle's)
    t.close()


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    import ctypes as C
    W, H = 128, 128
    h = heights(2, (32, 32))
    s = scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_viewshed((0.0, 0.0))
    s.set_shard(0, 1, 64)
    assert s.viewshed_info()["vertex"] is None                # (the refused call stored nothing)
    before = s.render_rgba().copy()
    xz, col = (C.c_float * 2)(0.1, 0.2), (C.c_uint8 * 4)(255, 0, 0, 128)
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_viewshed(t.t, 1, xz, 0.05, 0.0, 0.0, col, col, 0.02, 0.002) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    t.close()
    nan, inf = float("nan"), float("inf")
    # (eye_height, target_height, radius, softness, bias)
    for bad in ((-0.1, 0.0, 0.0, 0.02, 0.002), (0.05, -1.0, 0.0, 0.02, 0.002), (0.05, 0.0, -1.0, 0.02, 0.002), (0.05, 0.0, 0.0, 0.0, 0.002),
                (0.05, 0.0, 0.0, 0.02, -1.0), (nan, 0.0, 0.0, 0.02, 0.002), (0.05, inf, 0.0, 0.02, 0.002), (0.05, 0.0, nan, 0.02, 0.002),
                (0.05, 0.0, 0.0, inf, 0.002), (0.05, 0.0, 0.0, 0.02, nan)):
        t = terrain(W, H, 32, h)
        t.set_uniforms(uniforms(W, H))
        assert t.lib.vf_terrain_set_viewshed(t.t, 1, xz, bad[0], bad[1], bad[2], col, col, bad[3], bad[4]) == cabi.VF_ERR_INVALID, bad
        assert t.viewshed_info()["vertex"] is None and t.viewshed_info()["enabled"] is False
        t.close()
    t = terrain(W, H, 32, h)
    assert t.lib.vf_terrain_set_viewshed(t.t, 1, (C.c_float * 2)(nan, 0.0), 0.05, 0.0, 0.0, col, col, 0.02, 0.002) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_set_viewshed(t.t, 1, None, 0.05, 0.0, 0.0, col, col, 0.02, 0.002) == cabi.VF_ERR_INVALID
    out = np.zeros((32, 32), np.float32)
    assert t.lib.vf_terrain_read_viewshed_field(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID      # no observer yet
    t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene untinted)
    s.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, hidden_rgba=RED)
    tinted = s.render_rgba().copy()
    assert (tinted != before).any()
    with pytest.raises(RuntimeError, match="render_batch on a handle with a viewshed enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="viewshed enabled"):
        s.set_shard(0, 2, 64)
    with pytest.raises(ValueError, match="softness must be > 0"):
        s.set_viewshed(SCENE_OBSERVER, softness=0.0)
    assert np.array_equal(s.render_rgba(), tinted)
