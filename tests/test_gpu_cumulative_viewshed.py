"""Cumulative viewsheds on the GPU equal the CPU model (tests/cumulative_viewshed_model) bit for bit: the count field of
70 observers on grids inside one chunk, across a chunk boundary and over several chunks, with no radius, a small one, one that cuts
the chunks and one larger than the grid, at every batch size; over non-finite heights; through both entry points; the tinted frame
over two cameras, two sizes and both precisions with either colour alone and both; over shadows, ambient occlusion, a drape and under
the single observer's tint; under overlays; and nothing else moves -- the frame with the feature off or cleared, geometry buffers,
visibility, the single observer's viewshed, the scan counter of a resting scene, the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import cumulative_viewshed_model as cvm
import viewshed_model as vsm
from overlay_scenes import CAMERAS, apply, heights
from support import assert_field, assert_frame, bits, terrain, uniforms, vf, viridis  # noqa: F401
from test_gpu_viewshed import OBSERVERS, PARAMS
from viewshed_model import SCENE_OBSERVER, SCENE_PARAMS

RED, GREEN, BLUE = (255, 0, 0, 128), (64, 255, 96, 160), (0, 60, 255, 200)
FRAME_GRID = 257
# the frames' observers: raised above the noise of the test scene as the single observer of tests/test_gpu_viewshed.py is
FRAME_OBSERVERS = np.random.default_rng(12).uniform(-1.4, 1.4, (12, 2)).astype(np.float32)
FRAME_N = len(FRAME_OBSERVERS)


_counts = {}


def frame_count(u, h):
    """the model's count field of the frames' scene (it depends on the spacing and the exaggeration alone: computed once)"""
    key = (float(u[36]), float(u[38]), support.digest(h))
    if key not in _counts:
        _counts[key] = support.frozen(cvm.field(u, h, FRAME_GRID, FRAME_OBSERVERS, **SCENE_PARAMS)[0])
    return _counts[key]


def frame_scene(vf, W, H, h, cam="default", precision=None):
    s = vf.Scene(W, H, grid=FRAME_GRID)
    s.set_height_from_r32f(h)
    if precision is not None:
        s.set_shade_precision(precision)
    s.set_camera_look_at(*CAMERAS[cam])
    return s


# ---- the field ----

@pytest.mark.parametrize("grid", [130, 203, 257])
def test_field_equals_the_model_at_every_radius_and_batch_size(grid):
    observers = cvm.scene_observers()
    N = len(observers)
    assert N == 70 and np.array_equal(observers[:9], np.array(OBSERVERS, np.float32))
    h = heights(4, (97, 131))
    t = terrain(64, 64, grid, h)
    u = uniforms(64, 64, exag=0.6)
    t.set_uniforms(u)
    scans = 0
    # no radius; 11 to 21 cells; 47 / 74 / 94 cells: inside one chunk, across the boundary at step 64, two chunks; larger than the grid
    for radius in (None, 0.25, 1.1, 10.0):
        want, vertices, total = cvm.field(u, h, grid, observers, radius=radius, want_sum=True, **PARAMS)
        first = None
        for batch in (1, 4, 64, 70, 0):
            t.cumulative_viewshed_batch(batch)
            t.set_cumulative_viewshed(observers, enabled=False, radius=radius, **PARAMS)    # the field does not need the tint enabled
            got = t.cumulative_viewshed_field()
            scans += 1
            assert got.shape == (grid, grid) and got.dtype == np.float32
            assert_field(got, want, f"grid {grid} radius {radius} batch {batch}")
            first = got if first is None else first
            assert np.array_equal(bits(got), bits(first))
            info = t.cumulative_viewshed_info()
            assert info["batch"] == (batch or N) and info["observers"] == N and info["enabled"] is False
            assert info["radius"] == (None if radius is None else float(np.float32(radius)))
            assert info["vertices"].tolist() == [list(v) for v in vertices]
            assert t.cumulative_viewshed_scans() == scans
        if radius is None:
            assert (total == 0).sum() >= 0.05 * total.size and (total % 65536 != 0).sum() >= 0.25 * total.size and (total == N * 65536).any()
        elif radius < 5:
            assert (want < full).any() and (want <= full).all()
        else:
            assert np.array_equal(bits(want), bits(full))
        full = want if radius is None else full
    t.close()


def test_field_of_a_long_grid_with_three_observers():
    grid = 1025
    observers = [OBSERVERS[7], OBSERVERS[0], (0.9, 1.2)]
    h = heights(4, (97, 131))
    t = terrain(64, 64, grid, h)
    u = uniforms(64, 64, exag=0.6)
    t.set_uniforms(u)
    for radius, batch in ((None, 0), (None, 2), (1.1, 0), (1.1, 1)):       # Rc = 375.5 cells: six chunks of sixteen
        t.cumulative_viewshed_batch(batch)
        t.set_cumulative_viewshed(observers, enabled=False, radius=radius, **PARAMS)
        want = cvm.field(u, h, grid, observers, radius=radius, **PARAMS)[0]
        assert_field(t.cumulative_viewshed_field(), want, f"grid {grid} radius {radius} batch {batch}")
        assert (want > 0).any() and (want < 3).any()
    t.close()


def test_one_observer_gives_the_quantised_field_of_the_handles_own_viewshed():
    grid = 203
    h = heights(4, (97, 131))
    t = terrain(64, 64, grid, h)
    t.set_uniforms(uniforms(64, 64, exag=0.6))
    for obs in (OBSERVERS[7], OBSERVERS[1], OBSERVERS[8]):
        t.set_viewshed(obs, enabled=False, **PARAMS)
        seen = t.viewshed_field()
        t.set_cumulative_viewshed([obs], enabled=False, **PARAMS)
        got = t.cumulative_viewshed_field()
        assert np.array_equal(got.astype(np.float64), np.rint(seen.astype(np.float64) * 65536.0) / 65536.0), obs
        assert (seen < 1).any() and t.cumulative_viewshed_info()["vertices"].tolist() == [list(t.viewshed_info()["vertex"])]
        assert np.array_equal(bits(t.viewshed_field()), bits(seen))            # (the single observer's field is not disturbed)
    t.close()


def test_non_finite_heights_and_an_observer_on_a_hole():
    grid = 203
    h = heights(4, (97, 131)).copy()
    h[40:43, 60:62] = np.nan                                   # a hole
    h[70, 20] = np.inf
    u = uniforms(64, 64, exag=0.6)
    hv = vsm.shm.heights(u, h, grid)
    holes = np.argwhere(~np.isfinite(hv))
    assert 4 <= len(holes) < grid * grid // 50
    j, i = (int(c) for c in holes[len(holes) // 2])
    step = 3.0 / (grid - 1)
    on_hole = (-1.5 + i * step, -1.5 + j * step)
    assert vsm.observer_vertex(on_hole, 1.0, grid) == (i, j)
    observers = np.array(list(OBSERVERS[4:8]) + [on_hole], np.float32)
    t = terrain(64, 64, grid, h)
    t.set_uniforms(u)
    for radius in (None, 0.9):
        t.set_cumulative_viewshed(observers, enabled=False, radius=radius, **PARAMS)
        want, vertices, total = cvm.field(u, h, grid, observers, radius=radius, want_sum=True, **PARAMS)
        assert vertices[-1] == (i, j)
        assert_field(t.cumulative_viewshed_field(), want, f"holes, radius {radius}")
        blind = total - cvm.field(u, h, grid, observers[:-1], radius=radius, want_sum=True, **PARAMS)[2]
        assert set(np.unique(blind).tolist()) == ({65536} if radius is None else {0, 65536})      # the blind observer adds 1 in range
        if radius is None:
            assert (want[~np.isfinite(hv)] == len(observers)).all()             # a vertex without a height is seen by everybody
    t.close()


def test_field_into_device_memory_on_a_stream_of_the_callers():
    support.run_check("cumulative_viewshed_torch_check.py", "CUMULATIVE VIEWSHED TORCH OK")


# ---- frames ----

# both colours; the high colour alone; the low colour alone
TINTS = [dict(high_rgba=GREEN, low_rgba=RED), dict(high_rgba=GREEN, low_rgba=(0, 0, 0, 0)), dict(high_rgba=(64, 255, 96, 0), low_rgba=RED)]


@pytest.mark.parametrize("size", [(64, 64), (200, 120)])
@pytest.mark.parametrize("cam", ["default", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, size):
    W, H = size
    h = heights()
    for precision in ("exact", "fast"):
        s = frame_scene(vf, W, H, h, cam, precision)
        plain = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
        rgba, vis = support.oracle_frame(u, W, H, FRAME_GRID, h)
        if precision == "exact":
            assert np.array_equal(plain, rgba.reshape(H, W, 4))                # (the exact frame is the oracle's)
        cnt = frame_count(u, h)
        covered = vis != 0
        for tint in TINTS:
            s.set_cumulative_viewshed(FRAME_OBSERVERS, **SCENE_PARAMS, **tint)
            got = s.render_rgba()
            # the tint blends over the frame's own bytes: the oracle's in exact precision, the fast frame's in fast
            want, sv = cvm.frame(plain, vis, u, h, FRAME_GRID, cnt, FRAME_N, **tint)
            assert_frame(got, want, f"{precision} {cam} {size} {tint}")
            assert np.array_equal(sv >= 0, covered) and covered.any()
            assert (got != plain).any() and np.array_equal(got[~covered], plain[~covered])
            assert np.array_equal(s.render_rgba(), got)
        inner = sv[covered]
        assert ((inner > 0.02) & (inner < 0.98)).mean() > 0.3                  # (the tint is one of partial counts)
        assert_field(s.cumulative_viewshed_field(), cnt, "the scene's field")
        assert s.debug_cumulative_viewshed_scans() == 1                         # colours: no new field


def test_the_tint_lies_over_the_relight_passes_and_under_the_single_observers(vf):
    from shadow_model import SCENE_PARAMS as SHADOW_PARAMS, SCENE_SUN_DEG
    W, H = 200, 120
    h = heights()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 50, 4), dtype=np.uint8)
    single = dict(visible_rgba=(255, 255, 0, 90), hidden_rgba=(40, 0, 80, 120), radius=1.2)
    frames = {}
    for tinted in ("none", "cumulative", "both"):
        s = frame_scene(vf, W, H, h, "default", "exact")
        s.set_sun(*SCENE_SUN_DEG)
        s.set_shadows(True, **SHADOW_PARAMS)
        s.set_ambient_occlusion(True)
        s.set_drape(img, extent=(-1.0, -1.2, 0.9, 1.1), opacity=0.8)
        if tinted != "none":
            s.set_cumulative_viewshed(FRAME_OBSERVERS, **SCENE_PARAMS, high_rgba=BLUE, low_rgba=RED)
        if tinted == "both":
            s.set_viewshed(SCENE_OBSERVER, **SCENE_PARAMS, **single)
        frames[tinted] = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
    _, vis = support.oracle_frame(u, W, H, FRAME_GRID, h)
    plain = frame_scene(vf, W, H, h, "default", "exact").render_rgba()
    assert (frames["none"] != plain).any()
    under, _ = cvm.frame(frames["none"], vis, u, h, FRAME_GRID, frame_count(u, h), FRAME_N, high_rgba=BLUE, low_rgba=RED)
    assert (under != frames["none"]).any()
    assert_frame(frames["cumulative"], under, "tint over shadows, ambient occlusion and a drape")
    seen, v = vsm.field(u, h, FRAME_GRID, SCENE_OBSERVER, **SCENE_PARAMS)
    want, _ = vsm.frame(under, vis, u, h, FRAME_GRID, seen, v, **single)
    other, _ = cvm.frame(vsm.frame(frames["none"], vis, u, h, FRAME_GRID, seen, v, **single)[0], vis, u, h, FRAME_GRID, frame_count(u, h), FRAME_N,
                         high_rgba=BLUE, low_rgba=RED)
    assert (want != under).any() and (want != other).any()                      # (the order of the two tints shows)
    assert_frame(frames["both"], want, "the single observer's tint over the cumulative one")


def test_overlays_composite_over_the_tinted_frame(vf):
    import occlusion_model as ocm
    W, H = 200, 120
    h = heights()
    s = frame_scene(vf, W, H, h, "default", "exact")
    s.set_cumulative_viewshed(FRAME_OBSERVERS, **SCENE_PARAMS, high_rgba=GREEN, low_rgba=RED)
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 600
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.08, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(40)]
    calls = [("add_points", (pts,), dict(size_px=4.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)),
             ("add_lines", (paths,), dict(width_px=2.0, rgba=(0, 255, 0, 200), drape=True))]
    L = apply(vf, s, calls, ocm.Layers())
    rgba, vis = support.oracle_frame(u, W, H, FRAME_GRID, h)
    base, _ = cvm.frame(rgba, vis, u, h, FRAME_GRID, frame_count(u, h), FRAME_N, high_rgba=GREEN, low_rgba=RED)
    want = ocm.composite(base, vis, u, h, FRAME_GRID, L)
    got = s.render_rgba()
    assert (base != rgba.reshape(H, W, 4)).any() and (want != base).any()
    assert not np.array_equal(want, ocm.pm.composite(base, u, h, FRAME_GRID, L))   # (the occluding layer matters)
    assert_frame(got, want, "overlays over the tint")


# ---- what does not move ----

def test_nothing_else_moves_when_it_is_off_cleared_or_merely_set(vf):
    W, H = 200, 120
    h = heights(5)
    never = frame_scene(vf, W, H, h)
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    visib = never.debug_visibility().copy()
    single = dict(SCENE_PARAMS, hidden_rgba=RED)
    never.set_viewshed(SCENE_OBSERVER, **single)
    single_frame = never.render_rgba().copy()
    single_field = never.viewshed_field().copy()
    s = frame_scene(vf, W, H, h)
    info = s.cumulative_viewshed_info()
    assert info["enabled"] is False and info["vertices"] is None and info["observers"] == 0 and info["batch"] == 0
    assert np.array_equal(s.render_rgba(), want)              # before enabling
    s.set_cumulative_viewshed(FRAME_OBSERVERS, **SCENE_PARAMS, low_rgba=RED)
    tinted = s.render_rgba().copy()
    assert (tinted != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    assert np.array_equal(s.render_rgba(), tinted)
    s.set_cumulative_viewshed(FRAME_OBSERVERS, enabled=False, **SCENE_PARAMS, low_rgba=RED)
    assert np.array_equal(s.render_rgba(), want)              # off: the field is still there to be read
    assert s.cumulative_viewshed_field().shape == (FRAME_GRID, FRAME_GRID) and s.cumulative_viewshed_info()["vertices"].shape == (FRAME_N, 2)
    # the single observer's viewshed beside a cumulative one that is merely set: its field and its frames are the ones without
    s.set_viewshed(SCENE_OBSERVER, **single)
    assert np.array_equal(s.render_rgba(), single_frame)
    assert np.array_equal(bits(s.viewshed_field()), bits(single_field))
    s.clear_viewshed()
    s.set_cumulative_viewshed(FRAME_OBSERVERS, **SCENE_PARAMS, low_rgba=RED)
    assert np.array_equal(s.render_rgba(), tinted)
    s.clear_cumulative_viewshed()
    assert np.array_equal(s.render_rgba(), want)              # cleared
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert s.cumulative_viewshed_info()["vertices"] is None
    with pytest.raises(RuntimeError, match="no observers set"):
        s.cumulative_viewshed_field()
    sp = vf.TerrainSpike(160, 120, grid=48)
    sp.set_cumulative_viewshed([(0.2, 0.3), (-1.0, 1.0)])
    assert sp.cumulative_viewshed_field().shape == (48, 48) and 1.0 <= sp.cumulative_viewshed_field().max() <= 2.0
    assert sp.render_rgba().shape == (120, 160, 4)


def test_the_field_follows_its_inputs_and_rests_otherwise():
    W, H, grid = 160, 100, 130
    lut = viridis()
    h = heights(3)
    t = terrain(W, H, grid, h, lut)
    t.set_shade_precision(0)
    tint = dict(high_rgba=GREEN, low_rgba=RED)
    obs = FRAME_OBSERVERS[:5]
    t.set_cumulative_viewshed(obs, **SCENE_PARAMS, **tint)

    def check(u, hh, observers, what, params=SCENE_PARAMS, radius=None):
        import oracle
        t.render()
        got = t.read_rgba()
        rgba, vis = oracle.render_terrain(u, W, H, grid, hh, lut, want_vis=True, nthreads=8)
        cnt = cvm.field(u, hh, grid, observers, radius=radius, **params)[0]
        want, sv = cvm.frame(rgba, vis, u, hh, grid, cnt, len(observers), **tint)
        assert (want != rgba.reshape(H, W, 4)).any(), what
        assert_frame(got.reshape(H, W, 4), want, what)

    u = uniforms(W, H)
    t.set_uniforms(u)
    assert t.cumulative_viewshed_scans() == 0
    check(u, h, obs, "first frame")
    assert t.cumulative_viewshed_scans() == 1
    for _ in range(3):                                        # a resting scene pays once
        t.render()
    t.read_rgba()
    assert t.cumulative_viewshed_scans() == 1
    # what the field does not depend on: colours, camera, sun, observers that move inside their vertices' cells
    tint = dict(high_rgba=(0, 0, 255, 200), low_rgba=(20, 20, 20, 90))
    t.set_cumulative_viewshed(obs, **SCENE_PARAMS, **tint)
    u = uniforms(W, H, cam="fill", sun=(0.3, 0.8, -0.5))
    t.set_uniforms(u)
    check(u, h, obs, "new colours, camera and sun")
    assert t.cumulative_viewshed_scans() == 1
    step = 3.0 / (grid - 1)
    vertices = t.cumulative_viewshed_info()["vertices"]
    snapped = ((vertices * step - 1.5) + 0.2 * step).astype(np.float32)
    t.set_cumulative_viewshed(snapped, **SCENE_PARAMS, **tint)
    assert np.array_equal(t.cumulative_viewshed_info()["vertices"], vertices)
    t.render()
    assert t.cumulative_viewshed_scans() == 1
    # what it does depend on: the list of vertices (its order too: the key is the list), exaggeration, heights, a scan parameter, Rc
    t.set_cumulative_viewshed(obs[:4], **SCENE_PARAMS, **tint)
    check(u, h, obs[:4], "one observer fewer")
    assert t.cumulative_viewshed_scans() == 2
    u = uniforms(W, H, exag=1.6)
    t.set_uniforms(u)
    check(u, h, obs[:4], "new exaggeration")
    assert t.cumulative_viewshed_scans() == 3
    h2 = heights(9)
    t.set_height(h2)
    check(u, h2, obs[:4], "new heights")                       # (the setting survives a height upload)
    assert t.cumulative_viewshed_scans() == 4
    params = dict(SCENE_PARAMS)
    for k, (name, value) in enumerate((("eye_height", 1.4), ("target_height", 0.05), ("softness", 0.2), ("bias", 0.02))):
        params[name] = value
        t.set_cumulative_viewshed(obs[:4], **params, **tint)
        check(u, h2, obs[:4], f"new {name}", params=params)
        assert t.cumulative_viewshed_scans() == 5 + k
    t.set_cumulative_viewshed(obs[:4], radius=0.8, **params, **tint)
    check(u, h2, obs[:4], "a radius", params=params, radius=0.8)
    assert t.cumulative_viewshed_scans() == 9
    u = uniforms(W, H, exag=1.6, spacing=2.0)                  # the same world radius is half as many cells, from other vertices
    t.set_uniforms(u)
    check(u, h2, obs[:4], "a new spacing under a radius", params=params, radius=0.8)
    assert t.cumulative_viewshed_scans() == 10
    before = t.cumulative_viewshed_scans()
    assert t.cumulative_viewshed_stage(2) > 0 and t.cumulative_viewshed_scans() == before      # (diagnostic launches are not the handle's)
    t.close()


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    import ctypes as C
    W, H = 128, 128
    h = heights(2, (32, 32))
    s = frame_scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_cumulative_viewshed([(0.0, 0.0)])
    s.set_shard(0, 1, 64)
    assert s.cumulative_viewshed_info()["observers"] == 0     # (the refused call stored nothing)
    before = s.render_rgba().copy()
    xz, col = np.array([[0.1, 0.2], [0.3, -0.4]], np.float32), (C.c_uint8 * 4)(255, 0, 0, 128)
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_cumulative_viewshed(t.t, 1, xz.ctypes.data, 2, 0.05, 0.0, 0.0, col, col, 0.02, 0.002) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    t.close()
    nan, inf = float("nan"), float("inf")
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_cumulative_viewshed(xz, eye_height=0.3, **{k: v for k, v in PARAMS.items() if k != "eye_height"})
    t.render()
    kept, frame = t.cumulative_viewshed_info(), t.read_rgba().copy()

    def unchanged():
        now = t.cumulative_viewshed_info()
        assert now.keys() == kept.keys() and all(np.array_equal(now[k], kept[k]) for k in kept)
        t.render()
        assert np.array_equal(t.read_rgba(), frame) and t.cumulative_viewshed_scans() == 1

    # (eye_height, target_height, radius, softness, bias)
    for bad in ((-0.1, 0.0, 0.0, 0.02, 0.002), (0.05, -1.0, 0.0, 0.02, 0.002), (0.05, 0.0, -1.0, 0.02, 0.002), (0.05, 0.0, 0.0, 0.0, 0.002),
                (0.05, 0.0, 0.0, 0.02, -1.0), (nan, 0.0, 0.0, 0.02, 0.002), (0.05, inf, 0.0, 0.02, 0.002), (0.05, 0.0, nan, 0.02, 0.002),
                (0.05, 0.0, 0.0, inf, 0.002), (0.05, 0.0, 0.0, 0.02, nan)):
        assert t.lib.vf_terrain_set_cumulative_viewshed(t.t, 1, xz.ctypes.data, 2, bad[0], bad[1], bad[2], col, col, bad[3], bad[4]) == cabi.VF_ERR_INVALID, bad
    many = np.zeros((65536, 2), np.float32)
    for observers, count in ((xz, 0), (many, 65536), (np.array([[0.0, nan]], np.float32), 1), (np.array([[0.0, 0.0], [inf, 0.0]], np.float32), 2)):
        assert t.lib.vf_terrain_set_cumulative_viewshed(t.t, 1, observers.ctypes.data, count, 0.05, 0.0, 0.0, col, col, 0.02, 0.002) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_set_cumulative_viewshed(t.t, 1, None, 0, 0.05, 0.0, 0.0, col, col, 0.02, 0.002) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_set_cumulative_viewshed(t.t, 1, xz.ctypes.data, 2, 0.05, 0.0, 0.0, None, col, 0.02, 0.002) == cabi.VF_ERR_INVALID
    unchanged()
    t.close()
    t = terrain(W, H, 32, h)
    out = np.zeros((32, 32), np.float32)
    assert t.lib.vf_terrain_read_cumulative_viewshed_field(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID      # no observers yet
    t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene untinted)
    s.set_cumulative_viewshed(FRAME_OBSERVERS, **SCENE_PARAMS, low_rgba=RED)
    tinted = s.render_rgba().copy()
    scans = s.debug_cumulative_viewshed_scans()
    assert (tinted != before).any()
    with pytest.raises(RuntimeError, match="render_batch on a handle with a cumulative viewshed enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="cumulative viewshed enabled"):
        s.set_shard(0, 2, 64)
    with pytest.raises(ValueError, match="softness must be > 0"):
        s.set_cumulative_viewshed(FRAME_OBSERVERS, softness=0.0)
    with pytest.raises(ValueError, match="observers must hold 1 to 65535 rows"):
        s.set_cumulative_viewshed(np.zeros((0, 2), np.float32))
    assert np.array_equal(s.render_rgba(), tinted) and s.debug_cumulative_viewshed_scans() == scans
    assert s.cumulative_viewshed_info()["observers"] == FRAME_N
