"""Spill analysis on the GPU equals the CPU model (tests/spill_model) bit for bit: both fields on grids of one whole
tile, a tile of one column and one row, 3 x 3 tiles with edge tiles two vertices wide, and larger ones, from the border, one seed and a
seed list with a dry, a duplicate and an out-of-grid seed, through both entry points, with the model's counts; a serpentine channel
whose floor rises or falls and that crosses tile borders back and forth, at three group sizes; walls of non-finite heights on and
beside a tile border; the flood identity on the device; the tinted frame over three cameras, two sizes, both shade modes and both
precisions; over shadows, a drape and the flood's water; under the viewshed tint and the haze; under an occluding overlay layer; on a
supersampled handle; and nothing else moves -- the frame with the spill off or cleared, geometry buffers, visibility, the scan counter
of a resting scene, the refusals.  tests/test_spill_model.py holds these inputs to the conditions that keep the comparisons from being
vacuous."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import spill_model as spm
from spill_model import SCENE_SEEDS
from overlay_scenes import CAMERAS, GRID, heights, scene
from support import assert_field, assert_frame, bits, terrain, uniforms, vf, viridis  # noqa: F401

fdm, cm = spm.fdm, spm.cm
SHALLOW, DEEP = (96, 176, 224, 128), (16, 64, 160, 224)


def assert_fields(t, F, what):
    assert_field(t.spill_field(), F.spill, what + ": spill")
    assert_field(t.sink_depth_field(), F.sink, what + ": sink depth")
    info = t.spill_info()
    assert (info["reached_vertices"], info["sink_vertices"]) == (int(F.reached.sum()), int((F.sink > 0).sum())), (what, info)
    return info


# ---- the fields ----

@pytest.mark.parametrize("grid", spm.FIELD_GRIDS)
def test_fields_equal_the_model(grid):
    plain = heights(**spm.FIELD_TEXTURE)
    u = uniforms(64, 64, exag=0.6)
    tiles = spm.n_tiles(grid)
    for tex in (plain, spm.dry_texture(plain)):
        h = cm.surface(tex, grid)
        t = terrain(64, 64, grid, tex)
        t.set_uniforms(u)
        one, several = spm.field_seed_lists(h, grid)
        scans = 0
        for seeds in ("edges", one, several):
            what = f"grid {grid} seeds {seeds if isinstance(seeds, str) else len(seeds)} dry {tex is not plain}"
            t.set_spill(seeds, enabled=False)                  # the field does not need the spill enabled for drawing
            F = spm.field(u, tex, grid, seeds)
            info = assert_fields(t, F, what)
            scans += 1
            assert info["enabled"] is False and info["scans"] == scans            # (the second read found the field current)
            assert info["mode"] == ("edges" if isinstance(seeds, str) else "seeds")
            if F.vertices is None:
                assert info["vertices"] is None and info["seeds"] == 0
            else:
                assert np.array_equal(info["vertices"], F.vertices) and info["seeds"] == len(F.vertices)
            _, passes, _ = spm.tile_passes(h, "edges" if isinstance(seeds, str) else F.vertices)
            assert 2 <= info["passes"] <= passes, (what, info["passes"], passes)
            assert 1 <= info["tile_runs"] <= info["passes"] * tiles
            if grid >= 130:
                assert info["tile_runs"] < info["passes"] * tiles, (what, info)    # the flags let tiles leave
        t.close()


def test_fields_into_device_memory_on_a_stream_of_the_callers_and_the_flood_identity():
    support.run_check("spill_torch_check.py", "SPILL TORCH OK")


@pytest.mark.parametrize("slope", [+1.0, -1.0])
def test_a_serpentine_channel_at_three_group_sizes(slope):
    n = 130
    tex, start = spm.serpentine(n, slope)
    t = terrain(64, 64, n, tex)
    u = uniforms(64, 64)
    t.set_uniforms(u)
    seed = [spm.vertex_xz(start, n)]
    F = spm.field(u, tex, n, seed)
    assert F.vertices.tolist() == [list(start)] and F.reached.all()
    _, emulated, _ = spm.tile_passes(cm.surface(tex, n), F.vertices)
    assert emulated >= 8
    t.set_spill(seed, enabled=False)
    for k, group in enumerate((1, 7, 0)):
        t.spill_group(group)
        info = assert_fields(t, F, f"serpentine {slope}, group {group}")
        assert 2 <= info["passes"] <= emulated, (group, info["passes"], emulated)
        assert (info["group"] == group or not group) and info["scans"] == k + 1   # (a new group size computes the field again)
        assert info["tile_runs"] < info["passes"] * spm.n_tiles(n)
    assert t.spill_info()["group"] >= 1
    t.spill_group(0)
    t.spill_field()
    assert t.spill_info()["scans"] == 3                        # (the same group size: the field rests)
    t.spill_group(0, flags=False)                              # every tile in every pass: the same field
    info = assert_fields(t, F, f"serpentine {slope}, flags ignored")
    queued = -(-info["passes"] // info["group"]) * info["group"]                 # (the passes of the last group behind the fixpoint run too)
    assert info["tile_runs"] == queued * spm.n_tiles(n) and info["scans"] == 4
    t.spill_group(0)
    # from the far end and from the border
    for seeds in ([spm.vertex_xz((1, 127), n)], "edges"):
        t.set_spill(seeds, enabled=False)
        assert_fields(t, spm.field(u, tex, n, seeds), f"serpentine {slope} from {seeds}")
    t.close()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_walls_of_non_finite_heights_on_and_beside_a_tile_border(bad):
    n = 130
    tex = (0.2 * heights(7, (n, n))).astype(np.float32)
    tex[:, 60:70] = np.where(np.arange(60, 70) % 2 == 0, bad, tex[:, 60:70])    # walls on both sides of the tile border at 64
    tex[:, 64] = bad                                           # ... and on it
    tex[63:65, :20] = bad                                      # a wall along the other border, open at its end
    t = terrain(64, 64, n, tex)
    u = uniforms(64, 64)
    t.set_uniforms(u)
    for seeds in ([spm.vertex_xz((3, 3), n)], "edges"):
        t.set_spill(seeds, enabled=False)
        F = spm.field(u, tex, n, seeds)
        assert_fields(t, F, f"{bad} wall, seeds {seeds}")
        assert not F.reached[:, 64].any() and np.isfinite(t.sink_depth_field()).all()
    one = spm.field(u, tex, n, [spm.vertex_xz((3, 3), n)])
    assert one.reached[:, :60].sum() > 60 * n - 200 and not one.reached[:, 60:].any()   # the water stops at the first wall
    tex[77, 60:70] = 0.5                                       # a breach through all of them
    t.set_height(tex)
    assert_fields(t, spm.field(u, tex, n, "edges"), f"{bad} wall with a breach, from the border")   # (the setting survives the upload; the field does not)
    t.set_spill([spm.vertex_xz((3, 3), n)], enabled=False)
    F = spm.field(u, tex, n, [spm.vertex_xz((3, 3), n)])
    assert F.reached[:, 70:].all()
    assert_fields(t, F, f"{bad} wall with a breach")
    t.close()


# ---- the tinted frame ----

_fields = {}


def scene_field(u, h, seeds):
    key = (float(u[36]), support.digest(h), repr(seeds))
    if key not in _fields:
        _fields[key] = support.frozen(spm.field(u, h, GRID, seeds))
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
            s.set_spill(seeds, **tint)
            got = s.render_rgba()
            F = scene_field(u, h, seeds)
            # the tint blends over the frame's own bytes: the oracle's in exact precision, the fast frame's in fast
            want, d = spm.frame(plain, vis, u, h, GRID, F, **tint)
            assert_frame(got, want, f"{precision} {cam} {size} {mode} tint {k}")
            sink = d > 0
            assert sink.any() and (covered & ~sink).any()
            assert (got != plain).any() and np.array_equal(got[~sink], plain[~sink])
            assert np.array_equal(s.render_rgba(), got)
        assert_field(s.spill_field(), scene_field(u, h, SCENE_SEEDS[0]).spill, "the scene's field")
        assert_field(s.sink_depth_field(), scene_field(u, h, SCENE_SEEDS[0]).sink, "the scene's sink depth")
        assert s.debug_spill_scans() == 3                                        # new seeds: a new field; colours and depth_full: none


def test_the_tint_lies_over_shadows_a_drape_and_the_water_and_under_the_viewshed_tint_and_the_haze(vf):
    import supersample_model as ssm
    from shadow_model import SCENE_PARAMS as SHADOW_PARAMS, SCENE_SUN_DEG
    from viewshed_model import SCENE_OBSERVER, SCENE_PARAMS
    W, H = 640, 360
    h = heights()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 50, 4), dtype=np.uint8)
    view = dict(SCENE_PARAMS, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))
    haze = dict(density=0.25, rgba=(200, 215, 235, 255), start=1.0, falloff=0.5, base=-0.2, max_opacity=0.9)
    sink_tint = dict(shallow_rgba=(255, 224, 64, 160), deep_rgba=(160, 32, 16, 240), depth_full=0.2)
    frames = {}
    for stage in ("under", "sinks", "all"):
        s = scene(vf, W, H, h, "default", "exact")
        s.set_sun(*SCENE_SUN_DEG)
        s.set_shadows(True, **SHADOW_PARAMS)
        s.set_drape(img, extent=(-1.0, -1.2, 0.9, 1.1), opacity=0.8)
        if stage != "under":
            s.set_spill("edges", **sink_tint)                  # (set first: the order in the frame is not the order of the calls)
            s.set_flood(fdm.SCENE_LEVEL, SCENE_SEEDS[1])
        if stage == "all":
            s.set_viewshed(SCENE_OBSERVER, **view)
            s.set_haze(**haze)
        frames[stage] = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
    _, vis = support.oracle_frame(u, W, H, GRID, h)
    water, dw = fdm.frame(frames["under"], vis, u, h, GRID, fdm.field(u, h, GRID, fdm.SCENE_LEVEL, SCENE_SEEDS[1]))
    sinks, ds = spm.frame(water, vis, u, h, GRID, scene_field(u, h, "edges"), **sink_tint)
    plain = scene(vf, W, H, h, "default", "exact").render_rgba()
    assert (frames["under"] != plain).any() and (water != frames["under"]).any() and (sinks != water).any()
    assert ((dw > 0) & (ds > 0)).any()                         # pixels that take both tints: their order shows
    other, _ = fdm.frame(spm.frame(frames["under"], vis, u, h, GRID, scene_field(u, h, "edges"), **sink_tint)[0], vis, u, h, GRID,
                         fdm.field(u, h, GRID, fdm.SCENE_LEVEL, SCENE_SEEDS[1]))
    assert (other != sinks).any()
    assert_frame(frames["sinks"], sinks, "the sink tint over shadows, a drape and the water")
    want = ssm.chain(sinks, vis, u, h, GRID, viridis(), viewshed=dict(view, observer=SCENE_OBSERVER), haze=haze)
    assert (want != sinks).any()
    assert_frame(frames["all"], want, "the viewshed tint and the haze over the sink tint")


def test_an_occluding_overlay_layer_composites_over_the_tint(vf):
    W, H = 640, 360
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    s.set_spill("edges")
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 800
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    L = cm.Layers()
    s.add_points(pts, size_px=5.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)
    L.points(pts, size_px=5.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)
    rgba, vis = support.oracle_frame(u, W, H, GRID, h)
    base, d = spm.frame(rgba, vis, u, h, GRID, scene_field(u, h, "edges"))
    want = cm.ocm.composite(base, vis, u, h, GRID, L)
    got = s.render_rgba()
    assert (base != rgba).any() and (want != base).any()
    assert_frame(got, want, "an occluding layer over the sink tint")


def test_a_supersampled_handle_takes_the_tint_on_its_samples(vf):
    import supersample_model as ssm
    W, H, f, grid = 71, 45, 2, 130
    tex = heights(**spm.FIELD_TEXTURE)
    s = vf.Scene(W, H, grid=grid, supersample=f)
    s.set_height_from_r32f(tex)
    s.set_shade_precision("exact")
    s.set_camera_look_at(*CAMERAS["default"])
    plain = s.render_samples().copy()
    vis = s.debug_visibility().copy()
    u = s.debug_uniforms_f32()
    assert plain.shape == (f * H, f * W, 4) and vis.shape == (f * H, f * W)
    seeds = [spm.vertex_xz(spm.SEED_VERTEX, grid)]
    s.set_spill(seeds)
    F = spm.field(u, tex, grid, seeds)
    want, d = spm.frame(plain, vis, u, tex, grid, F)
    assert (d > 0).any() and ((vis != 0) & ~(d > 0)).any()
    frame = s.render_rgba().copy()
    assert_frame(s.render_samples(), want, "the samples over sinks")
    assert_frame(frame, ssm.resolve(want, f), "the resolved frame")
    assert_field(s.spill_field(), F.spill, "the supersampled handle's field")


# ---- nothing else moves ----

def test_the_frame_the_gbuffers_and_the_visibility_are_unchanged_when_off(vf):
    W, H = 640, 360
    h = heights(5)
    never = scene(vf, W, H, h)
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    visib = never.debug_visibility().copy()
    s = scene(vf, W, H, h)
    info = s.spill_info()
    assert info["enabled"] is False and info["mode"] is None and info["scans"] == 0 and info["tile_runs"] == 0
    assert (info["shallow_rgba"], info["deep_rgba"], info["depth_full"]) == (SHALLOW, DEEP, pytest.approx(0.1))
    assert set(info) == {"enabled", "mode", "seeds", "vertices", "shallow_rgba", "deep_rgba", "depth_full", "reached_vertices", "sink_vertices",
                         "passes", "scans", "group", "tile_runs"}
    assert np.array_equal(s.render_rgba(), want)              # before enabling
    with pytest.raises(RuntimeError, match="no spill set"):
        s.spill_field()
    with pytest.raises(RuntimeError, match="no spill set"):
        s.sink_depth_field()
    s.set_spill()
    assert s.spill_info()["mode"] == "edges"                  # the default mode
    tinted = s.render_rgba().copy()
    assert (tinted != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    assert np.array_equal(s.render_rgba(), tinted)
    s.set_spill("edges", enabled=False)
    assert np.array_equal(s.render_rgba(), want)              # off: the field is still there to be read
    assert s.spill_field().shape == (GRID, GRID) and s.spill_info()["mode"] == "edges"
    s.set_spill("edges")
    assert np.array_equal(s.render_rgba(), tinted)
    s.clear_spill()
    assert np.array_equal(s.render_rgba(), want)              # cleared
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    assert s.spill_info()["mode"] is None and s.spill_info()["reached_vertices"] == 0
    with pytest.raises(RuntimeError, match="no spill set"):
        s.spill_field()
    sp = vf.TerrainSpike(160, 120, grid=48)
    sp.set_spill([(0.2, 0.3)])
    assert sp.spill_field().shape == (48, 48) and sp.sink_depth_field().shape == (48, 48) and sp.spill_info()["vertices"].shape == (1, 2)
    assert sp.render_rgba().shape == (120, 160, 4)


def test_the_field_follows_its_inputs_and_rests_otherwise():
    W, H = 320, 200
    lut = viridis()
    h = heights(3)
    t = terrain(W, H, GRID, h, lut)
    t.set_shade_precision(0)
    seeds = [spm.vertex_xz(tuple(v), GRID) for v in fdm.seed_vertices(SCENE_SEEDS[1], 1.0, GRID).tolist()]   # (on their vertices: a nudge below stays inside the cell)
    tint = {}
    t.set_spill(seeds)

    def check(u, hh, sd, what):
        import oracle
        t.render()
        got = t.read_rgba()
        rgba, vis = oracle.render_terrain(u, W, H, GRID, hh, lut, want_vis=True, nthreads=8)
        F = spm.field(u, hh, GRID, sd)
        want, d = spm.frame(rgba.reshape(H, W, 4), vis, u, hh, GRID, F, **tint)
        assert (want != rgba.reshape(H, W, 4)).any(), what
        assert_frame(got.reshape(H, W, 4), want, what)

    u = uniforms(W, H)
    t.set_uniforms(u)
    assert t.spill_scans() == 0
    check(u, h, seeds, "first frame")
    assert t.spill_scans() == 1
    for _ in range(3):                                        # a resting scene pays once
        t.render()
    t.read_rgba()
    assert t.spill_scans() == 1
    # what the field does not depend on: colours, depth_full, camera, sun, exaggeration, a spacing or a nudge that leaves the seeds' vertices
    tint = dict(shallow_rgba=(0, 255, 255, 200), deep_rgba=(20, 20, 20, 90), depth_full=0.3)
    t.set_spill(seeds, **tint)
    check(u, h, seeds, "new colours and depth_full")
    u = uniforms(W, H, cam="fill", sun=(0.3, 0.8, -0.5), exag=1.6)
    t.set_uniforms(u)
    check(u, h, seeds, "new camera, sun and exaggeration")
    assert t.spill_scans() == 1
    step = 3.0 / (GRID - 1)
    nudged = [(x + 0.2 * step, z - 0.2 * step) for x, z in seeds]
    assert np.array_equal(fdm.seed_vertices(nudged, 1.0, GRID), fdm.seed_vertices(seeds, 1.0, GRID))
    t.set_spill(nudged, **tint)
    t.render()
    assert t.spill_scans() == 1                               # (seeds that move inside their vertices' cells)
    t.set_spill([(0.0, 0.0)], **tint)
    t.render()
    assert t.spill_scans() == 2                               # (the centre is another vertex ...)
    u = uniforms(W, H, cam="fill", spacing=1.7)
    t.set_uniforms(u)
    t.render()
    assert t.spill_scans() == 2                               # (... which stays the centre at any spacing)
    # what it does depend on
    t.set_spill(seeds, **tint)
    u = uniforms(W, H)
    t.set_uniforms(u)
    check(u, h, seeds, "back to the first seeds")
    assert t.spill_scans() == 3
    check(u, h, seeds, "nothing new")
    assert t.spill_scans() == 3
    t.set_spill("edges", **tint)
    check(u, h, "edges", "new mode")
    assert t.spill_scans() == 4
    h2 = heights(9)
    t.set_height(h2)
    check(u, h2, "edges", "new heights")                      # (the setting survives a height upload)
    assert t.spill_scans() == 5
    t.close()


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    import ctypes as C
    W, H = 128, 128
    h = heights(2, (32, 32))
    s = scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_spill()
    s.set_shard(0, 1, 64)
    assert s.spill_info()["mode"] is None                     # (the refused call stored nothing)
    before = s.render_rgba().copy()
    xz, col = (C.c_float * 4)(0.1, 0.2, -0.3, 0.4), (C.c_uint8 * 4)(255, 0, 0, 128)
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_spill(t.t, 1, 1, None, 0, col, col, 0.1) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    t.close()
    nan, inf = float("nan"), float("inf")
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    # (mode, seeds, count, depth_full)
    for bad in ((1, None, 0, 0.0), (1, None, 0, -1.0), (1, None, 0, nan), (1, None, 0, inf), (0, None, 0, 0.1), (3, None, 0, 0.1), (-1, xz, 2, 0.1),
                (2, xz, 0, 0.1), (2, xz, 65536, 0.1), (2, None, 2, 0.1), (2, (C.c_float * 4)(0.1, nan, 0.0, 0.0), 2, 0.1),
                (2, (C.c_float * 4)(0.1, 0.0, inf, 0.0), 2, 0.1)):
        assert t.lib.vf_terrain_set_spill(t.t, 1, bad[0], bad[1], bad[2], col, col, bad[3]) == cabi.VF_ERR_INVALID, bad
        info = t.spill_info()
        assert info["mode"] is None and info["enabled"] is False, bad
    assert t.lib.vf_terrain_set_spill(t.t, 1, 1, None, 0, None, col, 0.1) == cabi.VF_ERR_INVALID
    out = np.zeros((32, 32), np.float32)
    assert t.lib.vf_terrain_read_spill_field(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID          # no spill yet
    assert t.lib.vf_terrain_read_sink_depth(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_read_spill_seeds(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_debug_spill_group(t.t, 65) == cabi.VF_ERR_INVALID
    ms = (C.c_float * 2)()
    assert t.lib.vf_terrain_debug_spill_stage(t.t, 1, ms) == cabi.VF_ERR_INVALID
    t.render()                                                # the handle is usable
    assert t.read_rgba().size == H * W * 4
    t.set_spill([(0.1, 0.2), (-0.3, 0.4)])                    # ... and takes the spill
    t.render()
    assert t.spill_info()["seeds"] == 2 and t.spill_scans() == 1
    a, b = t.spill_stage(2)
    assert a > 0 and b > 0 and t.spill_scans() == 1           # (diagnostic launches are not the handle's)
    t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene as it was)
    s.set_spill("edges")
    tinted = s.render_rgba().copy()
    assert (tinted != before).any()
    with pytest.raises(RuntimeError, match="render_batch on a handle with the spill enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="spill enabled"):
        s.set_shard(0, 2, 64)
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_spill("edges")
    t.render()
    wet = t.read_rgba().copy()
    assert t.lib.vf_terrain_set_tile_shard(t.t, 0, 2, 3) == cabi.VF_ERR_INVALID           # tile-sharding a handle with the spill enabled
    assert "spill enabled" in t.lib.vf_last_error().decode()
    poses = np.concatenate([uniforms(W, H), uniforms(W, H, cam="fill")])
    outs = [np.zeros(H * W * 4, np.uint8) for _ in range(2)]
    ptrs = (C.c_void_p * 2)(*[o.ctypes.data for o in outs])
    assert t.lib.vf_terrain_render_batch_host(t.t, poses.ctypes.data, 2, ptrs) == cabi.VF_ERR_INVALID
    assert "render_batch on a handle with the spill enabled" in t.lib.vf_last_error().decode() and not outs[0].any()
    assert t.lib.vf_terrain_render_batch(t.t, poses.ctypes.data, 2, None, None) == cabi.VF_ERR_INVALID
    t.render()
    assert np.array_equal(t.read_rgba(), wet)                 # the refusals changed nothing
    t.close()
    with pytest.raises(ValueError, match="depth_full must be > 0"):
        s.set_spill(depth_full=0.0)
    with pytest.raises(ValueError, match="seeds must hold 1 to 65535 rows"):
        s.set_spill(np.zeros((0, 2)))
    with pytest.raises(ValueError, match='seeds must be "edges"'):
        s.set_spill("coast")
    with pytest.raises(ValueError, match='seeds must be "edges"'):
        s.set_spill(None)
    with pytest.raises(ValueError, match="seeds must be finite"):
        s.set_spill([(0.0, float("nan"))])
    assert np.array_equal(s.render_rgba(), tinted)
