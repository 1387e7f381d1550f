"""Atmospheric haze on the GPU equals the CPU model (tests/haze_model) bit for bit: the hazed frame and the opacity plane
over three cameras, two sizes that are no multiple of the pass's 32 x 8 region, both shade modes and both precisions, for uniform
haze, three falloffs (the difference branch of the height factor, both branches, the series), no start, a cap, a translucent colour
and the background on; at 1 x 1 and 130 x 3; over shadows, ambient occlusion, a drape and the three tints; under overlays; on
supersampled handles; into device memory on a caller's stream; and nothing else moves -- the frame with haze never set, disabled or
cleared, visibility, geometry buffers, pick, the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import haze_model as hzm
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from support import assert_frame, bits, vf, viridis  # noqa: F401

SIZES = [(96, 64), (71, 45)]
ORANGE = (255, 120, 40, 128)


def cases(cam):
    """the haze settings every frame test runs through: name -> set_haze's keywords"""
    P = hzm.SCENE_PARAMS[cam]
    out = {"uniform": dict(P), "no start": dict(P, start=0.0), "capped": dict(P, max_opacity=0.35), "translucent": dict(P, rgba=ORANGE),
           "background": dict(P, max_opacity=0.8, background=True), "translucent background": dict(P, rgba=ORANGE, background=True)}
    for f in hzm.SCENE_FALLOFFS:
        out[f"falloff {f}"] = dict(P, falloff=f, base=hzm.SCENE_BASE)
    return out


def assert_plane(got, want, what):
    assert got.shape == want.shape and got.dtype == np.float32, (what, got.shape, got.dtype)
    d = bits(got) != bits(want)
    assert not d.any(), f"{what}: {int(d.sum())} opacities differ, first at {np.argwhere(d)[:4].tolist()}: {got[d][:4]} against {want[d][:4]}"


@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_and_opacities_equal_the_model_in_both_precisions(vf, cam, size, mode):
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
        assert s.haze_info()["eye_y"] == float(hzm.eye_y(u))
        for name, kw in cases(cam).items():
            what = f"{precision} {cam} {size} {mode} {name}"
            s.set_haze(**kw)
            got = s.render_rgba().copy()
            # the haze blends over the frame's own bytes: the oracle's in exact precision, the fast frame's in fast
            want, a = hzm.frame(plain, vis, u, h, GRID, **kw)
            assert_frame(got, want, what)
            assert_plane(s.haze_opacity(), a, what)
            assert np.array_equal(s.render_rgba(), got)                          # (the opacity call left the frame alone)
            if covered.any():
                assert (a[covered] > 0).any() and (got != plain).any(), what
            if not kw.get("background"):
                assert np.array_equal(got[~covered], plain[~covered]), what
        s.set_haze(**cases(cam)["uniform"], enabled=False)
        assert np.array_equal(s.render_rgba(), plain)
        assert_plane(s.haze_opacity(), hzm.frame(plain, vis, u, h, GRID, **cases(cam)["uniform"])[1], "the plane of a disabled setting")


@pytest.mark.parametrize("size,cam", [((1, 1), "fill"), ((130, 3), "default"), ((130, 3), "near")])
def test_frames_of_one_pixel_and_of_three_rows(vf, size, cam):
    W, H = size
    h = heights()
    s = scene(vf, W, H, h, cam, "exact")
    plain = s.render_rgba().copy()
    u = s.debug_uniforms_f32()
    rgba, vis = support.oracle_frame(u, W, H, GRID, h)
    assert np.array_equal(plain, rgba)
    for name in ("no start", "falloff 0.3", "translucent background"):
        kw = cases(cam)[name]
        s.set_haze(**kw)
        want, a = hzm.frame(plain, vis, u, h, GRID, **kw)
        assert_frame(s.render_rgba(), want, f"{size} {cam} {name}")
        assert_plane(s.haze_opacity(), a, f"{size} {cam} {name}")
        assert (want != plain).any()


def test_background_haze_runs_on_a_frame_without_terrain(vf):
    W, H = 96, 64
    h = heights()
    s = vf.Scene(W, H, grid=GRID)
    s.set_height_from_r32f(h)
    s.set_camera_look_at((0.0, 3.0, 0.0), (0.0, 9.0, 0.5), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0)         # looking up, away from the ground
    plain = s.render_rgba().copy()
    assert (s.debug_visibility() == 0).all()
    s.set_haze(0.5, rgba=(255, 120, 40, 200), max_opacity=0.6, background=True)
    got = s.render_rgba().copy()
    a = np.float32(0.6) * (np.float32(200.0) / np.float32(255.0))
    want = plain.copy()
    for c in {tuple(p) for p in plain.reshape(-1, 4)[:, :3].tolist()}:
        want[(plain[..., :3] == c).all(axis=2), :3] = hzm.blend(c, (255, 120, 40, 200), a)
    assert_frame(got, want, "a frame of sky")
    assert (got != plain).any() and np.array_equal(got[..., 3], plain[..., 3])
    assert (s.haze_opacity() == a).all()
    s.set_haze(0.5, rgba=(255, 120, 40, 200), max_opacity=0.6)
    assert np.array_equal(s.render_rgba(), plain) and (s.haze_opacity() == 0).all()


def test_haze_lies_over_shadows_ambient_occlusion_a_drape_and_the_three_tints(vf):
    from shadow_model import SCENE_PARAMS as SHADOW_PARAMS, SCENE_SUN_DEG
    from viewshed_model import SCENE_OBSERVER, SCENE_PARAMS as VIEWSHED_PARAMS
    W, H = 96, 64
    h = heights()
    img = np.random.default_rng(3).integers(0, 256, (40, 50, 4), dtype=np.uint8)
    kw = cases("default")["falloff 4.0"]
    frames = {}
    for hazed in (False, True):
        s = scene(vf, W, H, h, "default", "exact")
        s.set_sun(*SCENE_SUN_DEG)
        s.set_shadows(True, **SHADOW_PARAMS)
        s.set_ambient_occlusion(True)
        s.set_drape(img, extent=(-1.0, -1.2, 0.9, 1.1), opacity=0.8)
        s.set_sun_exposure([(30.0, 120.0), (55.0, 200.0), (20.0, 300.0)])
        s.set_cumulative_viewshed([(0.4, 0.3), (-0.7, 0.5), (0.1, -0.9)], **VIEWSHED_PARAMS)
        s.set_viewshed(SCENE_OBSERVER, **VIEWSHED_PARAMS, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))
        if hazed:
            s.set_haze(**kw)
        frames[hazed] = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
    rgba, vis = support.oracle_frame(u, W, H, GRID, h)
    want, a = hzm.frame(frames[False], vis, u, h, GRID, **kw)
    assert (frames[False] != rgba).any() and (want != frames[False]).any()
    assert_frame(frames[True], want, "haze over shadows, ambient occlusion, a drape and the three tints")


def test_overlays_composite_over_the_hazed_frame_and_are_not_hazed(vf):
    import occlusion_model as ocm
    W, H = 96, 64
    h = heights()
    kw = cases("default")["background"]
    s = scene(vf, W, H, h, "default", "exact")
    s.set_haze(**kw)
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 60
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.2, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(12)]
    poly = [np.array([[-0.6, 0.05, -0.6], [0.7, 0.05, -0.5], [0.1, 0.05, 0.8]], np.float32)]
    calls = [("add_points", (pts,), dict(size_px=5.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)),
             ("add_lines", (paths,), dict(width_px=3.0, rgba=(0, 255, 0, 200), drape=True)),
             ("add_polygons", (poly,), dict(fill_rgba=(0, 90, 255, 160)))]
    L = apply(vf, s, calls, ocm.Layers())
    rgba, vis = support.oracle_frame(u, W, H, GRID, h)
    base, _ = hzm.frame(rgba, vis, u, h, GRID, **kw)
    want = ocm.composite(base, vis, u, h, GRID, L)
    assert (base != rgba).any() and (want != base).any()
    assert_frame(s.render_rgba(), want, "overlays over the haze")
    # ... and not the other way round: hazing the composited frame gives other bytes
    assert (hzm.frame(ocm.composite(rgba, vis, u, h, GRID, L), vis, u, h, GRID, **kw)[0] != want).any()


@pytest.mark.parametrize("f", [2, 3])
def test_supersampled_handles_haze_their_samples(vf, f):
    import oracle
    import supersample_model as ssm
    W, H = 37, 23
    h = heights()
    kw = cases("default")["falloff 4.0"]
    s = vf.Scene(W, H, grid=GRID, supersample=f)
    s.set_height_from_r32f(h)
    s.set_camera_look_at(*CAMERAS["default"])
    u = s.debug_uniforms_f32()
    plain_samples = s.render_samples().copy()
    rgba, vis = oracle.render_terrain(u, f * W, f * H, GRID, h, viridis(), want_vis=True, nthreads=8)
    assert np.array_equal(plain_samples, rgba.reshape(f * H, f * W, 4))
    s.set_haze(**kw)
    frame = s.render_rgba().copy()
    samples = s.render_samples()
    want, a = hzm.frame(plain_samples, vis, u, h, GRID, **kw)
    assert_frame(samples, want, f"samples, f = {f}")
    assert_frame(frame, ssm.resolve(want, f), f"the resolve of the hazed samples, f = {f}")
    assert_plane(s.haze_opacity(), a, f"the plane at the sample size, f = {f}")
    assert (want != plain_samples).any()
    s.clear_haze()
    assert np.array_equal(s.render_samples(), plain_samples)


def test_opacities_into_device_memory_on_a_stream_of_the_callers():
    support.run_check("haze_torch_check.py", "HAZE TORCH OK")


def test_the_frame_the_gbuffers_the_visibility_and_pick_are_unchanged(vf):
    W, H = 96, 64
    h = heights(5)
    never = scene(vf, W, H, h, precision="exact")
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    visib = never.debug_visibility().copy()
    pixels = [(0, 0), (W - 1, H - 1), (40, 30), (70, 50)]
    picked = never.pick(pixels)
    s = scene(vf, W, H, h, precision="exact")
    info = s.haze_info()
    assert info["enabled"] is False and info["density"] == 0.0 and info["falloff"] is None and info["rgba"] == (200, 215, 235, 255)
    assert np.array_equal(s.render_rgba(), want)              # never set
    assert (s.haze_opacity() == 0).all()
    kw = cases("default")["falloff 0.3"]
    s.set_haze(**kw, enabled=False)
    assert np.array_equal(s.render_rgba(), want)              # set, not enabled
    s.set_haze(**kw)
    hazed = s.render_rgba().copy()
    assert (hazed != want).any()
    info = s.haze_info()
    assert info["enabled"] is True and info["falloff"] == pytest.approx(0.3) and info["base"] == pytest.approx(hzm.SCENE_BASE) and info["background"] is False
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), visib)
    p = s.pick(pixels)
    for k in picked:
        assert np.array_equal(bits(p[k]), bits(picked[k])), k
    assert np.array_equal(s.render_rgba(), hazed)
    # the setting survives new heights and uniforms, and eye_y follows the uniforms
    u0 = s.debug_uniforms_f32()
    assert s.haze_info()["eye_y"] == float(hzm.eye_y(u0))
    s.set_camera_look_at(*CAMERAS["fill"])
    u1 = s.debug_uniforms_f32()
    assert s.haze_info()["eye_y"] == float(hzm.eye_y(u1)) != float(hzm.eye_y(u0))
    h2 = heights(9)
    s.set_height_from_r32f(h2)
    rgba, vis = support.oracle_frame(u1, W, H, GRID, h2)
    assert_frame(s.render_rgba(), hzm.frame(rgba, vis, u1, h2, GRID, **kw)[0], "new heights and camera")
    s.set_height_from_r32f(h)
    s.set_camera_look_at(*CAMERAS["default"])
    assert np.array_equal(s.render_rgba(), hazed)
    s.clear_haze()
    assert np.array_equal(s.render_rgba(), want)              # cleared
    assert s.haze_info()["enabled"] is False and s.haze_info()["density"] == 0.0
    sp = vf.TerrainSpike(160, 120, grid=48)
    before = sp.render_rgba().copy()
    sp.set_haze(0.8, falloff=0.5)
    assert sp.haze_opacity().shape == (120, 160) and (sp.render_rgba() != before).any()
    sp.clear_haze()
    assert np.array_equal(sp.render_rgba(), before)


def test_refusals_change_nothing(vf):
    import ctypes as C
    from vulkan_forge_amd import cabi
    W, H = 96, 64
    h = heights(2, (32, 32))
    s = scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_haze(0.5)
    s.set_shard(0, 1, 64)
    assert s.haze_info()["enabled"] is False and s.haze_info()["density"] == 0.0     # (the refused call stored nothing)
    before = s.render_rgba().copy()
    col = (C.c_uint8 * 4)(200, 215, 235, 255)
    import oracle
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)

    def terrain():
        t = cabi.Terrain(W, H, 32, np.zeros(1024, np.uint8))
        t.set_height(h)
        t.set_uniforms(u)
        return t
    t = terrain()
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_haze(t.t, 1, 0.5, col, 0.0, 0.0, 0.0, 1.0, 0) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    assert t.lib.vf_terrain_set_haze(t.t, 0, 0.5, col, 0.0, 0.0, 0.0, 1.0, 0) == cabi.VF_OK      # (stored, not enabled: allowed)
    t.close()
    nan, inf = float("nan"), float("inf")
    t = terrain()
    t.render()
    plain = t.read_rgba().copy()
    # (density, start, falloff, base, max_opacity) and a word of the message
    for bad, word in (((-0.1, 0.0, 0.0, 0.0, 1.0), "density"), ((nan, 0.0, 0.0, 0.0, 1.0), "density"), ((inf, 0.0, 0.0, 0.0, 1.0), "density"),
                      ((0.5, -1.0, 0.0, 0.0, 1.0), "start"), ((0.5, nan, 0.0, 0.0, 1.0), "start"), ((0.5, inf, 0.0, 0.0, 1.0), "start"),
                      ((0.5, 0.0, -2.0, 0.0, 1.0), "falloff"), ((0.5, 0.0, nan, 0.0, 1.0), "falloff"), ((0.5, 0.0, inf, 0.0, 1.0), "falloff"),
                      ((0.5, 0.0, 0.0, nan, 1.0), "base"), ((0.5, 0.0, 0.0, -inf, 1.0), "base"),
                      ((0.5, 0.0, 0.0, 0.0, 1.5), "max_opacity"), ((0.5, 0.0, 0.0, 0.0, -0.1), "max_opacity"), ((0.5, 0.0, 0.0, 0.0, nan), "max_opacity")):
        assert t.lib.vf_terrain_set_haze(t.t, 1, bad[0], col, bad[1], bad[2], bad[3], bad[4], 0) == cabi.VF_ERR_INVALID, bad
        assert word in t.lib.vf_last_error().decode(), (bad, t.lib.vf_last_error())
        assert t.haze_info()["enabled"] is False and t.haze_info()["density"] == 0.0
    assert t.lib.vf_terrain_set_haze(t.t, 1, 0.5, None, 0.0, 0.0, 0.0, 1.0, 0) == cabi.VF_ERR_INVALID
    assert "colour" in t.lib.vf_last_error().decode()
    t.render()
    assert np.array_equal(t.read_rgba(), plain)               # the handle is usable and unhazed
    t.set_haze(0.5, falloff=1.0)
    t.render()
    hazed_t = t.read_rgba().copy()
    assert (hazed_t != plain).any() and t.haze_stage(2) > 0.0
    with pytest.raises(cabi.VfError, match="haze enabled"):
        t.set_tile_shard(0, 2)
    with pytest.raises(cabi.VfError, match="haze enabled"):
        t.set_shard(0, 2, 64)
    uu = np.tile(u, 2)
    assert t.lib.vf_terrain_render_batch(t.t, uu.ctypes.data, 2, None, None) == cabi.VF_ERR_INVALID
    assert "render_batch on a handle with haze enabled is not supported" in t.lib.vf_last_error().decode()
    hosts = [np.zeros((H, W, 4), np.uint8) for _ in range(2)]
    ptrs = (C.c_void_p * 2)(*[x.ctypes.data for x in hosts])
    assert t.lib.vf_terrain_render_batch_host(t.t, uu.ctypes.data, 2, ptrs) == cabi.VF_ERR_INVALID
    assert "render_batch on a handle with haze enabled is not supported" in t.lib.vf_last_error().decode()
    t.render()
    assert np.array_equal(t.read_rgba(), hazed_t)
    t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene unhazed)
    s.set_haze(0.5)
    hazed = s.render_rgba().copy()
    assert (hazed != before).any()
    with pytest.raises(RuntimeError, match="render_batch on a handle with haze enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="haze enabled"):
        s.set_shard(0, 2, 64)
    with pytest.raises(ValueError, match=r"max_opacity must lie in \[0, 1\]"):
        s.set_haze(0.5, max_opacity=2.0)
    assert np.array_equal(s.render_rgba(), hazed)
