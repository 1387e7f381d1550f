"""Ambient occlusion on the GPU equals the CPU model (tests/ambient_model) bit for bit: the sky-view field on grids
that are no multiple of the tile, with reaches that cross none, one and two tile boundaries, for the default directions, an irregular
list, a single direction and a row of NaN heights, through both entry points; the frame over three cameras, two sizes, both shade
modes and both precisions, alone, with cast shadows and under overlays; the field is cached; and nothing else moves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import ambient_model as abm
import shadow_model as shm
from ambient_model import FIELD_CASES, IRREGULAR, SCENE_PARAMS, SCENE_SUN_DEG, scene_directions, scene_heights
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from support import assert_field, bits, terrain, uniforms, vf, viridis  # noqa: F401

SHADOW_PARAMS = abm.SCENE_SHADOWS


@pytest.mark.parametrize("grid,exag,reach,D", FIELD_CASES)
def test_field_equals_the_model(grid, exag, reach, D):
    from vulkan_forge_amd._ambient import directions
    h = heights(4, (97, 131))
    t = terrain(64, 64, grid, h)
    u = uniforms(64, 64, exag=exag)
    t.set_uniforms(u)
    dirs = directions(D)
    t.set_ambient_occlusion(False, reach=reach, directions=dirs)     # the field does not need ambient occlusion enabled for drawing
    got = t.sky_view_field()
    want = abm.field(u, h, grid, dirs, reach)
    assert got.shape == (grid, grid) and got.dtype == np.float32
    assert_field(got, want, f"grid {grid} reach {reach} D {D}")
    assert ((want > 0.1) & (want < 0.9)).mean() > 0.1                # (the comparison is not one of open sky)
    t.close()


def test_field_for_an_irregular_direction_list_and_a_row_of_nan_heights():
    grid, exag, reach = 203, 0.6, 16.0
    h = heights(4, (97, 131))
    t = terrain(64, 64, grid, h)
    u = uniforms(64, 64, exag=exag)
    t.set_uniforms(u)
    t.set_ambient_occlusion(False, reach=reach, directions=IRREGULAR)
    assert_field(t.sky_view_field(), abm.field(u, h, grid, IRREGULAR, reach), "irregular directions")
    hn = h.copy()
    hn[40, :] = np.nan                                               # a row of the texture: several vertex rows without a height
    t.set_height(hn)
    want = abm.field(u, hn, grid, IRREGULAR, reach)
    got = t.sky_view_field()
    assert_field(got, want, "a row of NaN heights")
    lost = ~np.isfinite(shm.heights(u, hn, grid))
    assert lost.any() and (got[lost] == 1.0).all() and (got[~lost] < 1.0).any()
    t.close()


def test_field_into_device_memory_on_a_stream_of_the_callers():
    support.run_check("ambient_torch_check.py", "AMBIENT TORCH OK")


def model_frame(u, W, H, h, mode, shadows=False):
    import oracle
    rgba, vis = oracle.render_terrain(u, W, H, GRID, h, viridis(), want_vis=True, nthreads=8,
                                      shade_mode=oracle.SHADE_SPEC_T32 if mode == "spec_t32" else oracle.SHADE_REFERENCE)
    sky = abm.field(u, h, GRID, scene_directions(), SCENE_PARAMS["reach"])
    lit = shm.field(u, h, GRID, **SHADOW_PARAMS) if shadows else None
    frame, mask = abm.frame(rgba, vis, u, h, GRID, viridis(), sky, SCENE_PARAMS["strength"], lit=lit, shade_mode=1 if mode == "spec_t32" else 0)
    return frame, mask, vis


def assert_frame(got, want, what, where=None):
    # byte for byte, at the pixels of the mask `where` if one is given
    support.assert_frame(got if where is None else np.where(where[..., None], got, want), want, what)


@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("size", [(96, 64), (256, 256)])
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, size, mode):
    W, H = size
    h = scene_heights()
    want = {}
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        s.set_sun(*SCENE_SUN_DEG)
        plain = s.render_rgba().copy()
        for shadows in (False, True):
            s.set_shadows(shadows, **SHADOW_PARAMS)
            s.set_ambient_occlusion(True, strength=SCENE_PARAMS["strength"], reach=SCENE_PARAMS["reach"], directions=scene_directions())
            got = s.render_rgba().copy()
            if shadows not in want:
                want[shadows] = model_frame(s.debug_uniforms_f32(), W, H, h, mode, shadows)
                frame, mask, vis = want[shadows]
                frac = mask.sum() / max(int((vis != 0).sum()), 1)
                print(f"{cam} {W}x{H} {mode} shadows={shadows}: {frac:.3f} of the covered pixels are written again")
                assert mask.any() and (shadows or 0.1 < frac < 0.9)
            frame, mask, vis = want[shadows]
            what = f"{precision} {cam} {size} {mode} shadows={shadows}"
            if precision == "exact":
                assert_frame(got, frame, what)
            else:                                             # rewritten pixels take the exact arithmetic, the others keep the fast frame's bytes
                assert_frame(got, frame, what + ", rewritten pixels", mask)
                assert_frame(got, plain, what + ", other pixels", ~mask)
            assert (got != plain).any()
            assert np.array_equal(s.render_rgba(), got)
        s.set_shadows(False)
        s.set_ambient_occlusion(False)
        assert np.array_equal(s.render_rgba(), plain)


def test_overlays_composite_over_the_ambient_frame(vf):
    W, H = 256, 256
    h = scene_heights()
    s = scene(vf, W, H, h, "default", "exact")
    s.set_sun(*SCENE_SUN_DEG)
    s.set_shadows(True, **SHADOW_PARAMS)
    s.set_ambient_occlusion(True, strength=SCENE_PARAMS["strength"], reach=SCENE_PARAMS["reach"], directions=scene_directions())
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 500
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.08, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(40)]
    poly = [np.array([[-0.6, 0.05, -0.6], [0.7, 0.05, -0.5], [0.1, 0.05, 0.8]], np.float32)]
    calls = [("add_points", (pts,), dict(size_px=5.0, rgba=(255, 0, 0, 200), drape=True)),
             ("add_lines", (paths,), dict(width_px=3.0, rgba=(0, 255, 0, 200), drape=True)),
             ("add_polygons", (poly,), dict(fill_rgba=(0, 90, 255, 160)))]
    import polygon_model as pm
    L = apply(vf, s, calls, pm.Layers())
    base, mask, _ = model_frame(u, W, H, h, "reference", shadows=True)
    want = pm.composite(base, u, h, GRID, L)
    got = s.render_rgba()
    assert mask.any() and (want != base).any()
    assert_frame(got, want, "overlays over ambient occlusion and shadows")


def test_the_field_is_cached(vf):
    W, H = 96, 64
    h = scene_heights()
    t = terrain(W, H, GRID, h, viridis())
    P = dict(strength=SCENE_PARAMS["strength"], reach=SCENE_PARAMS["reach"], directions=scene_directions())
    t.set_ambient_occlusion(True, **P)
    t.set_uniforms(uniforms(W, H, sun=shm.sun_vector(*SCENE_SUN_DEG)))
    assert t.ambient_scans() == 0
    t.render()
    first = t.read_rgba().copy()
    assert t.ambient_scans() == 1
    for _ in range(3):                                        # a resting scene pays once
        t.render()
    assert np.array_equal(t.read_rgba(), first) and t.ambient_scans() == 1
    t.set_uniforms(uniforms(W, H, sun=shm.sun_vector(40.0, 200.0)))                  # the sun
    t.render()
    t.set_uniforms(uniforms(W, H, cam="fill", sun=shm.sun_vector(40.0, 200.0)))      # the camera
    t.render()
    t.set_ambient_occlusion(True, **dict(P, strength=0.3))                           # strength
    t.render()
    assert (t.read_rgba() != first).any() and t.ambient_scans() == 1
    assert_field(t.sky_view_field(), abm.field(uniforms(W, H), h, GRID, scene_directions(), P["reach"]), "the cached field")
    assert t.ambient_scans() == 1
    t.set_uniforms(uniforms(W, H, exag=1.5))                                         # exaggeration
    t.render()
    assert t.ambient_scans() == 2
    t.set_height(scene_heights(9))                                                   # heights
    t.render()
    assert t.ambient_scans() == 3
    t.set_ambient_occlusion(True, **dict(P, reach=5.0))                              # reach
    t.render()
    assert t.ambient_scans() == 4
    t.set_ambient_occlusion(True, **dict(P, reach=5.0, directions=4))                # directions
    t.render()
    assert t.ambient_scans() == 5
    ms = t.ambient_stage(2)
    assert ms[0] > 0 and ms[1] > 0 and t.ambient_scans() == 5                        # (diagnostic launches are not the handle's)
    t.close()


def test_nothing_else_moves(vf):
    W, H = 256, 256
    h = scene_heights(5)
    never = scene(vf, W, H, h)
    never.set_sun(*SCENE_SUN_DEG)
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    never.set_shadows(True, **SHADOW_PARAMS)
    want_shadowed = never.render_rgba().copy()
    s = scene(vf, W, H, h)
    s.set_sun(*SCENE_SUN_DEG)
    assert s.debug_ambient_scans() == 0
    s.set_ambient_occlusion(True, strength=SCENE_PARAMS["strength"], reach=SCENE_PARAMS["reach"], directions=scene_directions())
    ambient = s.render_rgba().copy()
    assert (ambient != want).any() and s.debug_ambient_scans() == 1
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.render_rgba(), ambient)
    s.set_ambient_occlusion(False)
    assert np.array_equal(s.render_rgba(), want)              # after enable followed by disable
    s.set_shadows(True, **SHADOW_PARAMS)
    assert np.array_equal(s.render_rgba(), want_shadowed)     # the shadowed frame with ambient occlusion off
    assert s.sky_view_field().shape == (GRID, GRID)
    sp = vf.TerrainSpike(160, 120, grid=48)
    sp.set_ambient_occlusion(True)
    sky = sp.sky_view_field()
    assert sky.shape == (48, 48) and (sky >= 0).all() and (sky <= 1).all()
    assert sp.render_rgba().shape == (120, 160, 4)


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    W, H = 128, 128
    h = heights(2, (32, 32))
    s = scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_ambient_occlusion(True)
    s.set_shard(0, 1, 64)
    before = s.render_rgba().copy()
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_ambient(t.t, 1, 0.6, 64.0, 16, None) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    t.close()
    nan, inf = float("nan"), float("inf")
    zero = np.array([[1, 0], [0, 0]], np.float32)
    bad_dir = np.array([[1, 0], [nan, 1]], np.float32)
    for bad in ((1.5, 64.0, 16, None), (-0.1, 64.0, 16, None), (0.6, 0.5, 16, None), (0.6, 1025.0, 16, None), (0.6, 64.0, 0, None), (0.6, 64.0, 65, None),
                (nan, 64.0, 16, None), (0.6, inf, 16, None), (0.6, nan, 16, None), (0.6, 64.0, 2, zero.ctypes.data), (0.6, 64.0, 2, bad_dir.ctypes.data)):
        t = terrain(W, H, 32, h)
        t.set_uniforms(uniforms(W, H))
        t.set_ambient_occlusion(False, reach=2.0, directions=4)
        sky = t.sky_view_field()
        assert t.lib.vf_terrain_set_ambient(t.t, 1, *bad) == cabi.VF_ERR_INVALID, bad
        assert np.array_equal(t.sky_view_field(), sky) and t.ambient_scans() == 1
        t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene as it was)
    s.set_ambient_occlusion(True, reach=2.0)
    ambient = s.render_rgba().copy()
    with pytest.raises(RuntimeError, match="render_batch on a handle with ambient occlusion enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="ambient occlusion enabled"):
        s.set_shard(0, 2, 64)
    assert np.array_equal(s.render_rgba(), ambient)
