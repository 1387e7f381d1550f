"""Sun exposure on the GPU equals the CPU model (tests/sun_exposure_model) bit for bit: the exposure field of the 34
suns of the model's scene -- x-major, z-major, diagonal, axial, straight up, on and below the horizon, a weight of 0 -- on grids of
two chunks and a remainder, four chunks and a step into a fifth, with and without the incidence cosine, at every batch size; a long
grid; one sun by angles against the handle's own shadow field; over non-finite heights; through both entry points; the tinted frame
over two cameras, two sizes and both precisions with either colour alone and both; over shadows, ambient occlusion and a drape and
under both viewshed tints; under overlays; and nothing else moves -- the frame with the feature off, cleared or merely set, geometry
buffers, visibility, the other four fields, the scan counter of a resting scene, the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import cumulative_viewshed_model as cvm
import sun_exposure_model as sem
import viewshed_model as vsm
from overlay_scenes import CAMERAS, apply, heights
from support import assert_field, assert_frame, bits, terrain, uniforms, vf, viridis  # noqa: F401
from viewshed_model import SCENE_OBSERVER, SCENE_PARAMS as VIEW_PARAMS

shm = sem.shm
RED, GOLD, BLUE = (255, 0, 0, 128), (255, 208, 64, 160), (0, 60, 255, 200)
FRAME_GRID = 257
# the frames' suns: high ones, as the single sun of tests/test_gpu_shadows.py is -- the frames' scene is noise with slopes of about 100
FRAME_SUNS = np.stack([shm.sun_vector(62.0 + 2.0 * k, 11.0 + 30.0 * k) for k in range(12)] + [np.array((0.2, -0.1, 0.4), np.float32)]).astype(np.float32)
FRAME_WEIGHTS = np.append(np.random.default_rng(31).uniform(0.3, 1.0, 12), 1.0).astype(np.float32)
FRAME_PARAMS = dict(softness=0.1, bias=0.3)
FRAME_WTOT = sem.weight_total(FRAME_SUNS, FRAME_WEIGHTS)
SCENE_H = heights(4, (97, 131))


_wants = {}


def scene_want(grid, incidence, u):
    """the model's field of the 34 suns (computed once per grid and mode, and left unchanged)"""
    key = (grid, incidence)
    if key not in _wants:
        _wants[key] = sem.field(u, SCENE_H, grid, sem.SUNS, sem.WEIGHTS, incidence=incidence, want_sum=True)
    return _wants[key]


_fields = {}


def frame_field(u, h, incidence=False):
    """the model's exposure field of the frames' scene (it depends on the spacing and the exaggeration alone: computed once)"""
    key = (float(u[36]), float(u[38]), support.digest(h), incidence)
    if key not in _fields:
        _fields[key] = support.frozen(sem.field(u, h, FRAME_GRID, FRAME_SUNS, FRAME_WEIGHTS, incidence=incidence, **FRAME_PARAMS))
    return _fields[key]


def frame_scene(vf, W, H, h, cam="default", precision=None):
    s = vf.Scene(W, H, grid=FRAME_GRID)
    s.set_height_from_r32f(h)
    if precision is not None:
        s.set_shade_precision(precision)
    s.set_camera_look_at(*CAMERAS[cam])
    return s


# ---- the field ----

@pytest.mark.parametrize("incidence", [False, True])
@pytest.mark.parametrize("grid", [130, 203, 257])
def test_field_equals_the_model_at_every_batch_size(grid, incidence):
    N = len(sem.SUNS)
    assert N == 34
    t = terrain(64, 64, grid, SCENE_H)
    u = uniforms(64, 64, exag=0.6)
    t.set_uniforms(u)
    want, total = scene_want(grid, incidence, u)
    wtot = sem.weight_total(sem.SUNS, sem.WEIGHTS)
    first = None
    # 29 suns add something (30 counted, one of weight 0), 28 of them by a scan: batches of 1, of 4 (7 launches), of 5 (a last one of 3,
    # and one that holds x-major and z-major suns), all in one, and the default
    for k, batch in enumerate((1, 4, 5, 34, 0)):
        t.sun_exposure_batch(batch)
        t.set_sun_exposure(sem.SUNS, weights=sem.WEIGHTS, incidence=incidence, enabled=False)      # the field does not need the tint enabled
        got = t.sun_exposure_field()
        assert got.shape == (grid, grid) and got.dtype == np.float32
        assert_field(got, want, f"grid {grid} incidence {incidence} batch {batch}")
        first = got if first is None else first
        assert np.array_equal(bits(got), bits(first))
        info = t.sun_exposure_info()
        assert info["batch"] == (min(batch, 28) if batch else 28) and info["suns"] == N and info["counted"] == 30 and info["enabled"] is False
        assert info["incidence"] is incidence and np.float32(info["weight_total"]) == wtot
        assert t.sun_exposure_scans() == k + 1
    f = sem.fraction(want, wtot)
    if incidence:
        assert (f < 0.1).mean() >= 0.5 and (f >= 0.5).mean() >= 0.01 and f.max() >= 0.6
    else:
        assert (f < 0.1).mean() >= 0.3 and (f >= 0.5).mean() >= 0.25
    assert total.min() < total.max() // 4                      # (the straight-up sun reaches every vertex: no sum is 0)
    t.close()


def test_field_of_a_long_grid_with_three_suns():
    grid = 1025
    suns = np.array([(0.9, 0.35, 0.31), (-0.31, 0.4, 0.9), (-1.0, 0.5, 1.0)], np.float32)      # x-major, z-major, a diagonal
    w = np.array([1.0, 0.6, 0.8], np.float32)
    t = terrain(64, 64, grid, SCENE_H)
    u = uniforms(64, 64, exag=0.6)
    t.set_uniforms(u)
    for incidence, batch in ((False, 0), (False, 2), (True, 0), (True, 1)):
        t.sun_exposure_batch(batch)
        t.set_sun_exposure(suns, weights=w, incidence=incidence, enabled=False)
        want = sem.field(u, SCENE_H, grid, suns, w, incidence=incidence)
        assert_field(t.sun_exposure_field(), want, f"grid {grid} incidence {incidence} batch {batch}")
        assert (want == 0).any() and (want > 1).any()
    t.close()


def test_one_sun_by_angles_gives_the_quantised_field_of_the_handles_own_shadows(vf):
    grid = 203
    s = vf.Scene(64, 64, grid=grid)
    s.set_height_from_r32f(SCENE_H)
    s.set_camera_look_at(*CAMERAS["default"])
    for angles in ((35.0, 30.0), (20.0, 117.0), (50.0, -45.0), (12.5, 180.0)):
        s.set_sun(*angles)
        s.set_shadows(False, strength=1.0, softness=0.02, bias=0.002)
        lit = s.shadow_field()
        s.set_sun_exposure([angles], enabled=False)
        got = s.sun_exposure_field()
        assert np.array_equal(got.astype(np.float64), np.rint(lit.astype(np.float64) * 65536.0) / 65536.0), angles
        assert (lit < 1).any() and s.sun_exposure_info()["counted"] == 1
        u = s.debug_uniforms_f32()
        assert np.array_equal(bits(got), bits(sem.field(u, SCENE_H, grid, [u[32:35]])))           # (and the model's, from the handle's own vector)
        assert np.array_equal(bits(s.shadow_field()), bits(lit))                                   # (the shadow field is not disturbed)


def test_non_finite_heights():
    grid = 203
    h = SCENE_H.copy()
    h[40:43, 60:62] = np.nan                                   # a hole
    h[70, 20] = np.inf
    u = uniforms(64, 64, exag=0.6)
    hv = shm.heights(u, h, grid)
    holes = ~np.isfinite(hv)
    assert 4 <= holes.sum() < grid * grid // 50
    t = terrain(64, 64, grid, h)
    t.set_uniforms(u)
    for incidence in (False, True):
        t.set_sun_exposure(sem.SUNS, weights=sem.WEIGHTS, incidence=incidence, enabled=False)
        want, total = sem.field(u, h, grid, sem.SUNS, sem.WEIGHTS, incidence=incidence, want_sum=True)
        assert_field(t.sun_exposure_field(), want, f"holes, incidence {incidence}")
        if incidence:
            assert (total[holes] == 0).all()                   # no height, no slope, no cosine
        else:                                                  # a vertex without a height is lit by every counted sun
            assert (total[holes] == sum(int(np.rint(float(w) * 65536)) for w in sem.WEIGHTS[sem.counted(sem.SUNS)])).all()
    t.close()


def test_field_into_device_memory_on_a_stream_of_the_callers():
    support.run_check("sun_exposure_torch_check.py", "SUN EXPOSURE TORCH OK")


# ---- frames ----

# both colours; the high colour alone; the low colour alone
TINTS = [dict(high_rgba=GOLD, low_rgba=BLUE), dict(high_rgba=GOLD, low_rgba=(0, 0, 0, 0)), dict(high_rgba=(255, 208, 64, 0), low_rgba=BLUE)]


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
        e = frame_field(u, h)
        covered = vis != 0
        for tint in TINTS:
            s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, **FRAME_PARAMS, **tint)
            got = s.render_rgba()
            # the tint blends over the frame's own bytes: the oracle's in exact precision, the fast frame's in fast
            want, sv = sem.frame(plain, vis, u, h, FRAME_GRID, e, FRAME_WTOT, **tint)
            assert_frame(got, want, f"{precision} {cam} {size} {tint}")
            assert np.array_equal(sv >= 0, covered) and covered.any()
            assert (got != plain).any() and np.array_equal(got[~covered], plain[~covered])
            assert np.array_equal(s.render_rgba(), got)
        inner = sv[covered]
        assert ((inner > 0.02) & (inner < 0.98)).mean() > 0.3                  # (the tint is one of partial sums)
        assert_field(s.sun_exposure_field(), e, "the scene's field")
        assert s.debug_sun_exposure_scans() == 1                                # colours: no new field
        s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, incidence=True, **FRAME_PARAMS, **TINTS[0])
        want, _ = sem.frame(plain, vis, u, h, FRAME_GRID, frame_field(u, h, True), FRAME_WTOT, **TINTS[0])
        assert_frame(s.render_rgba(), want, f"{precision} {cam} {size} with incidence")
        assert s.debug_sun_exposure_scans() == 2


def test_the_tint_lies_over_the_relight_passes_and_under_both_viewshed_tints(vf):
    from shadow_model import SCENE_PARAMS as SHADOW_PARAMS, SCENE_SUN_DEG
    W, H = 200, 120
    h = heights()
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (40, 50, 4), dtype=np.uint8)
    single = dict(visible_rgba=(255, 255, 0, 90), hidden_rgba=(40, 0, 80, 120), radius=1.2)
    observers = np.random.default_rng(12).uniform(-1.4, 1.4, (6, 2)).astype(np.float32)
    cumulative = dict(high_rgba=(64, 255, 96, 120), low_rgba=(90, 0, 0, 60))
    frames = {}
    for tinted in ("none", "exposure", "all"):
        s = frame_scene(vf, W, H, h, "default", "exact")
        s.set_sun(*SCENE_SUN_DEG)
        s.set_shadows(True, **SHADOW_PARAMS)
        s.set_ambient_occlusion(True)
        s.set_drape(img, extent=(-1.0, -1.2, 0.9, 1.1), opacity=0.8)
        if tinted != "none":
            s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, **FRAME_PARAMS, high_rgba=GOLD, low_rgba=BLUE)
        if tinted == "all":
            s.set_cumulative_viewshed(observers, **VIEW_PARAMS, **cumulative)
            s.set_viewshed(SCENE_OBSERVER, **VIEW_PARAMS, **single)
        frames[tinted] = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
    _, vis = support.oracle_frame(u, W, H, FRAME_GRID, h)
    plain = frame_scene(vf, W, H, h, "default", "exact").render_rgba()
    assert (frames["none"] != plain).any()
    e = frame_field(u, h)
    under, _ = sem.frame(frames["none"], vis, u, h, FRAME_GRID, e, FRAME_WTOT, high_rgba=GOLD, low_rgba=BLUE)
    assert (under != frames["none"]).any()
    assert_frame(frames["exposure"], under, "tint over shadows, ambient occlusion and a drape")
    cnt = cvm.field(u, h, FRAME_GRID, observers, **VIEW_PARAMS)[0]
    seen, v = vsm.field(u, h, FRAME_GRID, SCENE_OBSERVER, **VIEW_PARAMS)
    mid, _ = cvm.frame(under, vis, u, h, FRAME_GRID, cnt, len(observers), **cumulative)
    want, _ = vsm.frame(mid, vis, u, h, FRAME_GRID, seen, v, **single)
    # the other order: the exposure tint over the two viewshed tints
    other = vsm.frame(cvm.frame(frames["none"], vis, u, h, FRAME_GRID, cnt, len(observers), **cumulative)[0], vis, u, h, FRAME_GRID, seen, v, **single)[0]
    other, _ = sem.frame(other, vis, u, h, FRAME_GRID, e, FRAME_WTOT, high_rgba=GOLD, low_rgba=BLUE)
    assert (want != mid).any() and (mid != under).any() and (want != other).any()              # (the order of the tints shows)
    assert_frame(frames["all"], want, "both viewshed tints over the sun exposure's")


def test_overlays_composite_over_the_tinted_frame(vf):
    import occlusion_model as ocm
    W, H = 200, 120
    h = heights()
    s = frame_scene(vf, W, H, h, "default", "exact")
    s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, **FRAME_PARAMS, high_rgba=GOLD, low_rgba=BLUE)
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 600
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.08, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(40)]
    calls = [("add_points", (pts,), dict(size_px=4.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)),
             ("add_lines", (paths,), dict(width_px=2.0, rgba=(0, 255, 0, 200), drape=True))]
    L = apply(vf, s, calls, ocm.Layers())
    rgba, vis = support.oracle_frame(u, W, H, FRAME_GRID, h)
    base, _ = sem.frame(rgba, vis, u, h, FRAME_GRID, frame_field(u, h), FRAME_WTOT, high_rgba=GOLD, low_rgba=BLUE)
    want = ocm.composite(base, vis, u, h, FRAME_GRID, L)
    got = s.render_rgba()
    assert (base != rgba.reshape(H, W, 4)).any() and (want != base).any()
    assert not np.array_equal(want, ocm.pm.composite(base, u, h, FRAME_GRID, L))   # (the occluding layer matters)
    assert_frame(got, want, "overlays over the tint")


# ---- what does not move ----

def test_nothing_else_moves_when_it_is_off_cleared_or_merely_set(vf):
    from shadow_model import SCENE_PARAMS as SHADOW_PARAMS
    W, H = 200, 120
    h = heights(5)
    observers = np.random.default_rng(12).uniform(-1.4, 1.4, (5, 2)).astype(np.float32)

    def others(s):
        """the other four fields of a handle"""
        s.set_shadows(False, **SHADOW_PARAMS)
        s.set_viewshed(SCENE_OBSERVER, enabled=False, **VIEW_PARAMS)
        s.set_cumulative_viewshed(observers, enabled=False, **VIEW_PARAMS)
        return [s.shadow_field().copy(), s.sky_view_field().copy(), s.viewshed_field().copy(), s.cumulative_viewshed_field().copy()]

    never = frame_scene(vf, W, H, h)
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    visib = never.debug_visibility().copy()
    fields = others(never)
    assert np.array_equal(never.render_rgba(), want)
    s = frame_scene(vf, W, H, h)
    info = s.sun_exposure_info()
    assert info == {"enabled": False, "suns": 0, "counted": 0, "weight_total": 0.0, "incidence": False, "batch": 0, "softness": float(np.float32(0.02)),
                    "bias": float(np.float32(0.002)), "high_rgba": GOLD, "low_rgba": (0, 0, 0, 0)}
    assert np.array_equal(s.render_rgba(), want)              # before enabling
    s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, **FRAME_PARAMS, low_rgba=BLUE)
    tinted = s.render_rgba().copy()
    assert (tinted != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    assert np.array_equal(s.render_rgba(), tinted)
    s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, enabled=False, **FRAME_PARAMS, low_rgba=BLUE)
    assert np.array_equal(s.render_rgba(), want)              # off: the field is still there to be read
    assert s.sun_exposure_field().shape == (FRAME_GRID, FRAME_GRID) and s.sun_exposure_info()["suns"] == len(FRAME_SUNS)
    # the other four fields beside a sun exposure that is merely set are the ones without
    for got, ref, name in zip(others(s), fields, ("lit", "sky", "seen", "count")):
        assert np.array_equal(bits(got), bits(ref)), name
    assert np.array_equal(s.render_rgba(), want)
    s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, **FRAME_PARAMS, low_rgba=BLUE)
    assert np.array_equal(s.render_rgba(), tinted)
    s.clear_sun_exposure()
    assert np.array_equal(s.render_rgba(), want)              # cleared
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert s.sun_exposure_info() == info
    with pytest.raises(RuntimeError, match="no suns set"):
        s.sun_exposure_field()
    for got, ref, name in zip(others(s), fields, ("lit", "sky", "seen", "count")):
        assert np.array_equal(bits(got), bits(ref)), name
    sp = vf.TerrainSpike(160, 120, grid=48)
    sp.set_sun_exposure([(40.0, 20.0), (-3.0, 100.0), (25.0, 200.0)], weights=[1.0, 1.0, 0.5])
    assert sp.sun_exposure_field().shape == (48, 48) and 0.0 < sp.sun_exposure_field().max() <= 1.5 and sp.sun_exposure_info()["counted"] == 2
    assert sp.sun_exposure_info()["weight_total"] == 1.5 and sp.render_rgba().shape == (120, 160, 4)


def test_the_field_follows_its_inputs_and_rests_otherwise():
    W, H, grid = 160, 100, 130
    lut = viridis()
    h = heights(3)
    t = terrain(W, H, grid, h, lut)
    t.set_shade_precision(0)
    state = dict(suns=FRAME_SUNS[:5].copy(), weights=FRAME_WEIGHTS[:5].copy(), incidence=False, high_rgba=GOLD, low_rgba=BLUE, **FRAME_PARAMS)

    def put(**change):
        state.update(change)
        t.set_sun_exposure(state["suns"], **{k: v for k, v in state.items() if k != "suns"})

    def check(u, hh, what):
        import oracle
        t.render()
        got = t.read_rgba()
        rgba, vis = oracle.render_terrain(u, W, H, grid, hh, lut, want_vis=True, nthreads=8)
        e = sem.field(u, hh, grid, state["suns"], state["weights"], incidence=state["incidence"], softness=state["softness"], bias=state["bias"])
        want, sv = sem.frame(rgba, vis, u, hh, grid, e, sem.weight_total(state["suns"], state["weights"]), high_rgba=state["high_rgba"],
                             low_rgba=state["low_rgba"])
        assert (want != rgba.reshape(H, W, 4)).any(), what
        assert_frame(got.reshape(H, W, 4), want, what)

    put()
    u = uniforms(W, H)
    t.set_uniforms(u)
    assert t.sun_exposure_scans() == 0
    check(u, h, "first frame")
    assert t.sun_exposure_scans() == 1
    for _ in range(3):                                        # a resting scene pays once
        t.render()
    t.read_rgba()
    assert t.sun_exposure_scans() == 1
    # what the field does not depend on: colours, the camera, the handle's own sun
    put(high_rgba=(0, 0, 255, 200), low_rgba=(20, 20, 20, 90))
    u = uniforms(W, H, cam="fill", sun=(0.3, 0.8, -0.5))
    t.set_uniforms(u)
    check(u, h, "new colours, camera and sun")
    assert t.sun_exposure_scans() == 1
    # what it does depend on: a sun, a weight, incidence, softness, bias, exaggeration, spacing, heights
    suns = state["suns"].copy()
    suns[2] = shm.sun_vector(70.0, 200.0)
    scans = 1
    w = state["weights"].copy()
    w[1] = 0.125
    for what, change in (("another sun", dict(suns=suns)), ("one sun fewer", dict(suns=suns[:4], weights=state["weights"][:4])),
                         ("another weight", dict(weights=w[:4])), ("incidence", dict(incidence=True)), ("softness", dict(softness=0.2)),
                         ("bias", dict(bias=0.2))):
        put(**change)
        check(u, h, what)
        scans += 1
        assert t.sun_exposure_scans() == scans, what
    u = uniforms(W, H, exag=1.6)
    t.set_uniforms(u)
    check(u, h, "new exaggeration")
    assert t.sun_exposure_scans() == scans + 1
    u = uniforms(W, H, exag=1.6, spacing=2.0)
    t.set_uniforms(u)
    check(u, h, "new spacing")
    assert t.sun_exposure_scans() == scans + 2
    h2 = heights(9)
    t.set_height(h2)
    check(u, h2, "new heights")                               # (the setting survives a height upload)
    assert t.sun_exposure_scans() == scans + 3
    assert t.sun_exposure_stage(2) > 0 and t.sun_exposure_scans() == scans + 3      # (diagnostic launches are not the handle's)
    t.close()


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    import ctypes as C
    W, H = 128, 128
    h = heights(2, (32, 32))
    s = frame_scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_sun_exposure([(40.0, 20.0)])
    s.set_shard(0, 1, 64)
    assert s.sun_exposure_info()["suns"] == 0                 # (the refused call stored nothing)
    before = s.render_rgba().copy()
    xyz, w, col = np.array([[0.5, 0.6, 0.2], [-0.3, 0.8, -0.4]], np.float32), np.array([1.0, 0.5], np.float32), (C.c_uint8 * 4)(255, 0, 0, 128)
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_sun_exposure(t.t, 1, xyz.ctypes.data, w.ctypes.data, 2, 0, 0.02, 0.002, col, col) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    t.close()
    nan, inf = float("nan"), float("inf")
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_sun_exposure(xyz, weights=w, softness=0.3, bias=0.1, low_rgba=RED)
    t.render()
    kept, frame = t.sun_exposure_info(), t.read_rgba().copy()

    def unchanged():
        assert t.sun_exposure_info() == kept
        t.render()
        assert np.array_equal(t.read_rgba(), frame) and t.sun_exposure_scans() == 1

    for soft, bias in ((0.0, 0.002), (-1.0, 0.002), (0.02, -1.0), (nan, 0.002), (inf, 0.002), (0.02, nan), (0.02, inf)):
        assert t.lib.vf_terrain_set_sun_exposure(t.t, 1, xyz.ctypes.data, w.ctypes.data, 2, 0, soft, bias, col, col) == cabi.VF_ERR_INVALID, (soft, bias)
    many = np.ones((65536, 3), np.float32)
    for suns, count in ((xyz, 0), (many, 65536), (np.array([[0.0, nan, 1.0]], np.float32), 1), (np.array([[0.0, 1.0, 0.0], [inf, 1.0, 0.0]], np.float32), 2)):
        assert t.lib.vf_terrain_set_sun_exposure(t.t, 1, suns.ctypes.data, None, count, 0, 0.02, 0.002, col, col) == cabi.VF_ERR_INVALID
    for bad in ((1.0, -0.01), (1.5, 1.0), (nan, 1.0), (1.0, inf)):
        bw = np.array(bad, np.float32)
        assert t.lib.vf_terrain_set_sun_exposure(t.t, 1, xyz.ctypes.data, bw.ctypes.data, 2, 0, 0.02, 0.002, col, col) == cabi.VF_ERR_INVALID, bad
    assert t.lib.vf_terrain_set_sun_exposure(t.t, 1, None, None, 2, 0, 0.02, 0.002, col, col) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_set_sun_exposure(t.t, 1, xyz.ctypes.data, None, 2, 0, 0.02, 0.002, None, col) == cabi.VF_ERR_INVALID
    unchanged()
    t.close()
    t = terrain(W, H, 32, h)
    out = np.zeros((32, 32), np.float32)
    assert t.lib.vf_terrain_read_sun_exposure_field(t.t, out.ctypes.data) == cabi.VF_ERR_INVALID      # no suns yet
    assert "no suns set" in t.lib.vf_last_error().decode()
    t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene untinted)
    s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS, **FRAME_PARAMS, low_rgba=BLUE)
    tinted = s.render_rgba().copy()
    scans = s.debug_sun_exposure_scans()
    kept = s.sun_exposure_info()
    assert (tinted != before).any()
    with pytest.raises(RuntimeError, match="render_batch on a handle with sun exposure enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="sun exposure enabled"):
        s.set_shard(0, 2, 64)
    with pytest.raises(ValueError, match="softness must be > 0"):
        s.set_sun_exposure(FRAME_SUNS, softness=0.0)
    with pytest.raises(ValueError, match="suns must hold 1 to 65535 rows"):
        s.set_sun_exposure(np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match=r"weights must be finite and lie in \[0, 1\]"):
        s.set_sun_exposure(FRAME_SUNS, weights=FRAME_WEIGHTS * 2)
    assert np.array_equal(s.render_rgba(), tinted) and s.debug_sun_exposure_scans() == scans
    assert s.sun_exposure_info() == kept
