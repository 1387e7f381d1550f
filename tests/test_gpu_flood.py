"""Flood analysis on the GPU equals the CPU model (tests/flood_model) bit for bit: the field on grids of one whole
tile, a tile of one column and one row, 3 x 3 tiles with edge tiles two vertices wide, and larger ones, from one seed, a seed list
with a dry, a duplicate and an out-of-grid seed, the border and everywhere, through both entry points, with the model's counts; a
serpentine channel that crosses tile borders back and forth, at three group sizes; a NaN wall across a tile border; the tinted frame
over three cameras, two sizes, both shade modes and both precisions; over shadows and a drape; under the viewshed tint and the haze;
under overlays with the shoreline's contour on top; on a supersampled handle; and nothing else moves -- the frame with the flood off
or cleared, geometry buffers, visibility, the scan counter of a resting scene, the refusals.  tests/test_flood_model.py holds these
inputs to the conditions that keep the comparisons from being vacuous."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import flood_model as fdm
from flood_model import SCENE_LEVEL, SCENE_SEEDS
from overlay_scenes import CAMERAS, GRID, heights, scene
from support import assert_field, assert_frame, bits, terrain, uniforms, vf, viridis  # noqa: F401

cm = fdm.cm
SHALLOW, DEEP = (96, 176, 224, 128), (16, 64, 160, 224)


def assert_info(info, F, what):
    assert (info["flooded_vertices"], info["wettable_vertices"]) == (int(F.flooded.sum()), int(F.wet.sum())), (what, info)


# ---- the field ----

@pytest.mark.parametrize("grid", fdm.FIELD_GRIDS)
def test_field_equals_the_model(grid):
    tex = heights(**fdm.FIELD_TEXTURE)
    h = cm.surface(tex, grid)
    t = terrain(64, 64, grid, tex)
    u = uniforms(64, 64, exag=0.6)
    t.set_uniforms(u)
    scans = 0
    for q in fdm.FIELD_QUANTILES:
        level = fdm.field_level(h, q)
        one, several = fdm.field_seed_lists(h, level, grid)
        for seeds in (one, several, "edges", None):
            what = f"grid {grid} quantile {q} seeds {seeds if seeds is None or isinstance(seeds, str) else len(seeds)}"
            t.set_flood(level, seeds, enabled=False)          # the field does not need the flood enabled for drawing
            got = t.flood_field()
            scans += 1
            F = fdm.field(u, tex, grid, level, seeds)
            assert_field(got, F.depth, what)
            info = t.flood_info()
            assert_info(info, F, what)
            assert info["enabled"] is False and info["scans"] == scans and info["level"] == np.float32(level)
            assert info["mode"] == ("everywhere" if seeds is None else seeds if isinstance(seeds, str) else "seeds")
            if F.vertices is None:
                assert info["vertices"] is None and info["seeds"] == 0
            else:
                assert np.array_equal(info["vertices"], F.vertices) and info["seeds"] == len(F.vertices)
            if seeds is None:
                assert info["passes"] == 0
            else:
                _, passes = fdm.tile_passes(F.wet, fdm.sources(F.wet, "edges" if isinstance(seeds, str) else F.vertices))
                assert 2 <= info["passes"] <= passes, (what, info["passes"], passes)
    t.close()


def test_field_into_device_memory_on_a_stream_of_the_callers():
    support.run_check("flood_torch_check.py", "FLOOD TORCH OK")


def test_a_serpentine_channel_at_three_group_sizes():
    n = 130
    tex, start, count = fdm.serpentine(n)
    t = terrain(64, 64, n, tex)
    u = uniforms(64, 64)
    t.set_uniforms(u)
    seed = [fdm.vertex_xz(start, n)]
    F = fdm.field(u, tex, n, 0.0, seed)
    assert F.vertices.tolist() == [list(start)] and int(F.flooded.sum()) == count
    _, emulated = fdm.tile_passes(F.wet, fdm.sources(F.wet, F.vertices))
    assert emulated >= 8
    t.set_flood(0.0, seed, enabled=False)
    seen = []
    for k, group in enumerate((1, 7, 0)):
        t.flood_group(group)
        got = t.flood_field()
        info = t.flood_info()
        assert_field(got, F.depth, f"serpentine, group {group}")
        assert_info(info, F, f"serpentine, group {group}")
        assert 2 <= info["passes"] <= emulated, (group, info["passes"], emulated)
        assert (info["group"] == group or not group) and info["scans"] == k + 1                     # (a new group size computes the field again)
        seen.append(info["passes"])
    assert t.flood_info()["group"] >= 1
    t.flood_group(0)
    t.flood_field()
    assert t.flood_info()["scans"] == 3                        # (the same group size: the field rests)
    # the far end alone floods the same channel; a seed on a wall floods nothing
    t.set_flood(0.0, [fdm.vertex_xz((1, 127), n)], enabled=False)
    assert_field(t.flood_field(), F.depth, "serpentine from its far end")
    t.set_flood(0.0, [fdm.vertex_xz((0, 0), n)], enabled=False)
    assert not t.flood_field().any() and t.flood_info()["flooded_vertices"] == 0 and t.flood_info()["passes"] == 1
    t.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_wall_of_non_finite_heights_across_a_tile_border(bad):
    n = 130
    tex = np.full((n, n), -1.0, np.float32)                    # (with the analytic relief of +-0.5 every vertex lies below 0)
    tex[:, 60:70] = np.where(np.arange(60, 70) % 2 == 0, bad, -1.0)[None, :]    # walls on both sides of the tile border at 64
    tex[:, 64] = bad                                           # ... and on it
    t = terrain(64, 64, n, tex)
    u = uniforms(64, 64)
    t.set_uniforms(u)
    for seeds in ([fdm.vertex_xz((3, 3), n)], "edges", None):
        t.set_flood(0.0, seeds, enabled=False)
        F = fdm.field(u, tex, n, 0.0, seeds)
        got = t.flood_field()
        assert_field(got, F.depth, f"{bad} wall, seeds {seeds}")
        assert_info(t.flood_info(), F, f"{bad} wall")
        assert np.isfinite(got).all() and not F.wet[:, 64].any()
    one = fdm.field(u, tex, n, 0.0, [fdm.vertex_xz((3, 3), n)])
    assert one.flooded[:, :60].all() and not one.flooded[:, 60:].any()          # the water stops at the first wall
    tex[77, 60:70] = -1.0                                      # a breach through all of them
    t.set_height(tex)
    t.set_flood(0.0, [fdm.vertex_xz((3, 3), n)], enabled=False)
    F = fdm.field(u, tex, n, 0.0, [fdm.vertex_xz((3, 3), n)])
    assert F.flooded[:, 70:].all()
    assert_field(t.flood_field(), F.depth, f"{bad} wall with a breach")
    t.close()


# ---- the tinted frame ----

_fields = {}


def scene_field(u, h, seeds):
    key = (float(u[36]), support.digest(h), repr(seeds))
    if key not in _fields:
        _fields[key] = support.frozen(fdm.field(u, h, GRID, SCENE_LEVEL, seeds))
    return _fields[key]


# the defaults from the border; other colours and a shallower depth_full from the seed list; the deep colour alone
TINTS = [dict(seeds=SCENE_SEEDS[0]), dict(seeds=SCENE_SEEDS[1], shallow_rgba=(255, 255, 255, 200), deep_rgba=(0, 0, 96, 255), depth_full=0.03),
         dict(seeds=SCENE_SEEDS[0], shallow_rgba=(0, 0, 0, 0), deep_rgba=DEEP, depth_full=0.25)]


@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("size", [(640, 360), (257, 131)])
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, size, mode):
    W, H = size
    h = heights()
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        plain = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
        rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
        if precision == "exact":
            assert np.array_equal(plain, rgba)                                   # (the exact frame is the oracle's)
        covered = vis != 0
        for k, tint in enumerate(TINTS):
            tint = dict(tint)
            seeds = tint.pop("seeds")
            s.set_flood(SCENE_LEVEL, seeds, **tint)
            got = s.render_rgba()
            F = scene_field(u, h, seeds)
            # the water blends over the frame's own bytes: the oracle's in exact precision, the fast frame's in fast
            want, d = fdm.frame(plain, vis, u, h, GRID, F, **tint)
            assert_frame(got, want, f"{precision} {cam} {size} {mode} tint {k}")
            water = d > 0
            assert water.any() and (covered & ~water).any()
            assert (got != plain).any() and np.array_equal(got[~water], plain[~water])
            assert np.array_equal(s.render_rgba(), got)
        assert_field(s.flood_field(), scene_field(u, h, SCENE_SEEDS[0]).depth, "the scene's field")
        assert s.debug_flood_scans() == 3                                        # new seeds: a new field; colours and depth_full: none


def test_the_water_lies_over_shadows_and_a_drape_and_under_the_viewshed_tint_and_the_haze(vf):
    import supersample_model as ssm
    from shadow_model import SCENE_PARAMS as SHADOW_PARAMS, SCENE_SUN_DEG
    from viewshed_model import SCENE_OBSERVER, SCENE_PARAMS
    W, H = 640, 360
    h = heights()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 50, 4), dtype=np.uint8)
    view = dict(SCENE_PARAMS, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))
    haze = dict(density=0.25, rgba=(200, 215, 235, 255), start=1.0, falloff=0.5, base=-0.2, max_opacity=0.9)
    frames = {}
    for stage in ("under", "water", "all"):
        s = scene(vf, W, H, h, "default", "exact")
        s.set_sun(*SCENE_SUN_DEG)
        s.set_shadows(True, **SHADOW_PARAMS)
        s.set_drape(img, extent=(-1.0, -1.2, 0.9, 1.1), opacity=0.8)
        if stage != "under":
            s.set_flood(SCENE_LEVEL, SCENE_SEEDS[0])
        if stage == "all":
            s.set_viewshed(SCENE_OBSERVER, **view)
            s.set_haze(**haze)
        frames[stage] = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
    _, vis = support.oracle_frame(u, W, H, GRID, h)
    F = scene_field(u, h, SCENE_SEEDS[0])
    water, d = fdm.frame(frames["under"], vis, u, h, GRID, F)
    plain = scene(vf, W, H, h, "default", "exact").render_rgba()
    assert (frames["under"] != plain).any() and (water != frames["under"]).any()
    assert_frame(frames["water"], water, "water over shadows and a drape")
    want = ssm.chain(water, vis, u, h, GRID, viridis(), viewshed=dict(view, observer=SCENE_OBSERVER), haze=haze)
    assert (want != water).any()
    assert_frame(frames["all"], want, "the viewshed tint and the haze over the water")


def test_overlays_and_the_shoreline_contour_composite_over_the_water(vf):
    W, H = 640, 360
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    s.set_flood(SCENE_LEVEL, SCENE_SEEDS[0])
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 800
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    L = cm.Layers()
    s.add_points(pts, size_px=5.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)
    L.points(pts, size_px=5.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)
    s.add_contours(np.asarray([SCENE_LEVEL], np.float32), width_px=1.5, rgba=(255, 255, 255, 255))
    L.contours(h, GRID, u, [SCENE_LEVEL], width_px=1.5, rgba=(255, 255, 255, 255))
    rgba, vis = support.oracle_frame(u, W, H, GRID, h)
    F = scene_field(u, h, SCENE_SEEDS[0])
    base, d = fdm.frame(rgba, vis, u, h, GRID, F)
    want = cm.ocm.composite(base, vis, u, h, GRID, L)
    got = s.render_rgba()
    assert (base != rgba).any() and (want != base).any()
    assert_frame(got, want, "overlays and the shoreline over the water")


def test_a_supersampled_handle_takes_the_water_on_its_samples(vf):
    import supersample_model as ssm
    W, H, f, grid = 71, 45, 2, 130
    tex = heights(**fdm.FIELD_TEXTURE)
    s = vf.Scene(W, H, grid=grid, supersample=f)
    s.set_height_from_r32f(tex)
    s.set_shade_precision("exact")
    s.set_camera_look_at(*CAMERAS["default"])
    plain = s.render_samples().copy()
    vis = s.debug_visibility().copy()
    u = s.debug_uniforms_f32()
    assert plain.shape == (f * H, f * W, 4) and vis.shape == (f * H, f * W)
    surface = cm.surface(tex, grid)
    level = fdm.field_level(surface)
    seeds = [fdm.vertex_xz(fdm.SEED_VERTEX, grid)]
    s.set_flood(level, seeds)
    F = fdm.field(u, tex, grid, level, seeds)
    want, d = fdm.frame(plain, vis, u, tex, grid, F)
    assert (d > 0).any() and ((vis != 0) & ~(d > 0)).any()
    frame = s.render_rgba().copy()
    assert_frame(s.render_samples(), want, "the samples under water")
    assert_frame(frame, ssm.resolve(want, f), "the resolved frame")
    assert_field(s.flood_field(), F.depth, "the supersampled handle's field")


# ---- nothing else moves ----

def test_the_frame_the_gbuffers_and_the_visibility_are_unchanged_when_off(vf):
    W, H = 640, 360
    h = heights(5)
    never = scene(vf, W, H, h)
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    visib = never.debug_visibility().copy()
    s = scene(vf, W, H, h)
    info = s.flood_info()
    assert info["enabled"] is False and info["level"] is None and info["mode"] is None and info["scans"] == 0
    assert (info["shallow_rgba"], info["deep_rgba"], info["depth_full"]) == (SHALLOW, DEEP, pytest.approx(0.1))
    assert np.array_equal(s.render_rgba(), want)              # before enabling
    with pytest.raises(RuntimeError, match="no flood set"):
        s.flood_field()
    s.set_flood(SCENE_LEVEL, "edges")
    tinted = s.render_rgba().copy()
    assert (tinted != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    assert np.array_equal(s.render_rgba(), tinted)
    s.set_flood(SCENE_LEVEL, "edges", enabled=False)
    assert np.array_equal(s.render_rgba(), want)              # off: the field is still there to be read
    assert s.flood_field().shape == (GRID, GRID) and s.flood_info()["level"] == pytest.approx(SCENE_LEVEL)
    s.set_flood(SCENE_LEVEL, "edges")
    assert np.array_equal(s.render_rgba(), tinted)
    s.clear_flood()
    assert np.array_equal(s.render_rgba(), want)              # cleared
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    assert s.flood_info()["level"] is None and s.flood_info()["flooded_vertices"] == 0
    with pytest.raises(RuntimeError, match="no flood set"):
        s.flood_field()
    sp = vf.TerrainSpike(160, 120, grid=48)
    sp.set_flood(0.1, [(0.2, 0.3)])
    assert sp.flood_field().shape == (48, 48) and sp.flood_info()["vertices"].shape == (1, 2)
    assert sp.render_rgba().shape == (120, 160, 4)


def test_the_field_follows_its_inputs_and_rests_otherwise():
    W, H = 320, 200
    lut = viridis()
    h = heights(3)
    t = terrain(W, H, GRID, h, lut)
    t.set_shade_precision(0)
    seeds = [fdm.vertex_xz(tuple(v), GRID) for v in fdm.seed_vertices(SCENE_SEEDS[1], 1.0, GRID).tolist()]   # (on their vertices: a nudge below stays inside the cell)
    tint = {}
    t.set_flood(SCENE_LEVEL, seeds)

    def check(u, hh, level, sd, what):
        import oracle
        t.render()
        got = t.read_rgba()
        rgba, vis = oracle.render_terrain(u, W, H, GRID, hh, lut, want_vis=True, nthreads=8)
        F = fdm.field(u, hh, GRID, level, sd)
        want, d = fdm.frame(rgba.reshape(H, W, 4), vis, u, hh, GRID, F, **tint)
        assert (want != rgba.reshape(H, W, 4)).any(), what
        assert_frame(got.reshape(H, W, 4), want, what)

    u = uniforms(W, H)
    t.set_uniforms(u)
    assert t.flood_scans() == 0
    check(u, h, SCENE_LEVEL, seeds, "first frame")
    assert t.flood_scans() == 1
    for _ in range(3):                                        # a resting scene pays once
        t.render()
    t.read_rgba()
    assert t.flood_scans() == 1
    # what the field does not depend on: colours, depth_full, camera, sun, exaggeration, a spacing or a nudge that leaves the seeds' vertices
    tint = dict(shallow_rgba=(0, 255, 255, 200), deep_rgba=(20, 20, 20, 90), depth_full=0.3)
    t.set_flood(SCENE_LEVEL, seeds, **tint)
    check(u, h, SCENE_LEVEL, seeds, "new colours and depth_full")
    u = uniforms(W, H, cam="fill", sun=(0.3, 0.8, -0.5), exag=1.6)
    t.set_uniforms(u)
    check(u, h, SCENE_LEVEL, seeds, "new camera, sun and exaggeration")
    assert t.flood_scans() == 1
    step = 3.0 / (GRID - 1)
    nudged = [(x + 0.2 * step, z - 0.2 * step) for x, z in seeds]
    assert np.array_equal(fdm.seed_vertices(nudged, 1.0, GRID), fdm.seed_vertices(seeds, 1.0, GRID))
    t.set_flood(SCENE_LEVEL, nudged, **tint)
    t.render()
    assert t.flood_scans() == 1                               # (seeds that move inside their vertices' cells)
    t.set_flood(SCENE_LEVEL, [(0.0, 0.0)], **tint)
    t.render()
    assert t.flood_scans() == 2                               # (the centre is another vertex ...)
    u = uniforms(W, H, cam="fill", spacing=1.7)
    t.set_uniforms(u)
    t.render()
    assert t.flood_scans() == 2                               # (... which stays the centre at any spacing)
    # what it does depend on
    t.set_flood(SCENE_LEVEL, seeds, **tint)
    u = uniforms(W, H)
    t.set_uniforms(u)
    check(u, h, SCENE_LEVEL, seeds, "back to the first seeds")
    assert t.flood_scans() == 3
    check(u, h, SCENE_LEVEL, seeds, "nothing new")
    assert t.flood_scans() == 3
    t.set_flood(0.2, seeds, **tint)
    check(u, h, 0.2, seeds, "new level")
    assert t.flood_scans() == 4
    t.set_flood(0.2, "edges", **tint)
    check(u, h, 0.2, "edges", "new mode")
    assert t.flood_scans() == 5
    h2 = heights(9)
    t.set_height(h2)
    check(u, h2, 0.2, "edges", "new heights")                 # (the setting survives a height upload)
    assert t.flood_scans() == 6
    t.close()


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    import ctypes as C
    W, H = 128, 128
    h = heights(2, (32, 32))
    s = scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_flood(0.0)
    s.set_shard(0, 1, 64)
    assert s.flood_info()["level"] is None                    # (the refused call stored nothing)
    before = s.render_rgba().copy()
    xz, col = (C.c_float * 4)(0.1, 0.2, -0.3, 0.4), (C.c_uint8 * 4)(255, 0, 0, 128)
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_flood(t.t, 1, 0.0, 0, None, 0, col, col, 0.1) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    t.close()
    nan, inf = float("nan"), float("inf")
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    # (level, mode, seeds, count, depth_full)
    for bad in ((nan, 0, None, 0, 0.1), (inf, 0, None, 0, 0.1), (-inf, 1, None, 0, 0.1), (0.0, 0, None, 0, 0.0), (0.0, 0, None, 0, -1.0),
                (0.0, 0, None, 0, nan), (0.0, 0, None, 0, inf), (0.0, 3, None, 0, 0.1), (0.0, -1, xz, 2, 0.1), (0.0, 2, xz, 0, 0.1),
                (0.0, 2, xz, 65536, 0.1), (0.0, 2, None, 2, 0.1), (0.0, 2, (C.c_float * 4)(0.1, nan, 0.0, 0.0), 2, 0.1),
                (0.0, 2, (C.c_float * 4)(0.1, 0.0, inf, 0.0), 2, 0.1)):
        assert t.lib.vf_terrain_set_flood(t.t, 1, bad[0], bad[1], bad[2], bad[3], col, col, bad[4]) == cabi.VF_ERR_INVALID, bad
        info = t.flood_info()
        assert info["level"] is None and info["enabled"] is False, bad
    assert t.lib.vf_terrain_set_flood(t.t, 1, 0.0, 0, None, 0, None, col, 0.1) == cabi.VF_ERR_INVALID
    out = np.zeros((32, 32), np.float32)
    assert t.lib.vf_terrain_read_flood_field(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID          # no flood yet
    assert t.lib.vf_terrain_read_flood_seeds(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_debug_flood_group(t.t, 65) == cabi.VF_ERR_INVALID
    t.render()                                                # the handle is usable
    assert t.read_rgba().size == H * W * 4
    t.set_flood(0.0, [(0.1, 0.2), (-0.3, 0.4)])               # ... and takes a flood
    t.render()
    assert t.flood_info()["seeds"] == 2 and t.flood_scans() == 1
    t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene dry)
    s.set_flood(0.1, "edges")
    tinted = s.render_rgba().copy()
    assert (tinted != before).any()
    with pytest.raises(RuntimeError, match="render_batch on a handle with a flood enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="flood enabled"):
        s.set_shard(0, 2, 64)
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_flood(0.1, "edges")
    t.render()
    wet = t.read_rgba().copy()
    assert t.lib.vf_terrain_set_tile_shard(t.t, 0, 2, 3) == cabi.VF_ERR_INVALID           # tile-sharding a handle with a flood enabled
    assert "flood enabled" in t.lib.vf_last_error().decode()
    poses = np.concatenate([uniforms(W, H), uniforms(W, H, cam="fill")])
    outs = [np.zeros(H * W * 4, np.uint8) for _ in range(2)]
    ptrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    assert t.lib.vf_terrain_render_batch_host(t.t, poses.ctypes.data, 2, ptrs) == cabi.VF_ERR_INVALID
    assert "render_batch on a handle with a flood enabled" in t.lib.vf_last_error().decode() and not outs[0].any()
    assert t.lib.vf_terrain_render_batch(t.t, poses.ctypes.data, 2, None, None) == cabi.VF_ERR_INVALID
    t.render()
    assert np.array_equal(t.read_rgba(), wet)                 # the refusals changed nothing
    t.close()
    with pytest.raises(ValueError, match="depth_full must be > 0"):
        s.set_flood(0.1, depth_full=0.0)
    with pytest.raises(ValueError, match="level must be finite"):
        s.set_flood(nan)
    with pytest.raises(ValueError, match="seeds must hold 1 to 65535 rows"):
        s.set_flood(0.1, np.zeros((0, 2)))
    with pytest.raises(ValueError, match='seeds must be None, "edges"'):
        s.set_flood(0.1, "coast")
    assert np.array_equal(s.render_rgba(), tinted)
