"""Hazed overlay layers on the GPU equal the CPU model (tests/overlay_haze_model) bit for bit, applied to the same
handle's hazed frame drawn without overlays and the oracle's visibility of it: points (circles and squares, draped and free, 1, 6 and
64 px, per-feature translucent colours) and polylines (three caps, widths 1 and 5, draped and free, a segment across the whole depth
range, a path through the near plane) over three cameras and two sizes under uniform haze, three falloffs, a cap and a translucent
haze colour; a contour layer; hazed and unhazed layers interleaved over polygons; hazed layers that occlude, or stand beside one that
does; a bin with more primitives than one sort window; 1 x 1 and 130 x 3 frames; supersampled handles; the flag switched off and on;
new haze parameters and new heights without touching the layers; haze off in every way; and the refusals.
tests/test_overlay_haze_model.py holds the frames drawn here to the conditions that keep these comparisons from being vacuous."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import overlay_haze_model as ohm
import overlay_haze_scenes as sc
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from support import assert_frame, vf  # noqa: F401

ocm = ohm.ocm
F32 = np.float32
TRIANGLE = [np.array([[-0.9, 0.05, -0.8], [1.0, 0.05, -0.6], [0.1, 0.05, 1.1]], F32)]


_vis = {}


def oracle_vis(u, W, H, h):
    """the oracle's visibility: computed once per case, shared, left unchanged"""
    import oracle
    key = (u.tobytes(), W, H, support.digest(h))
    if key not in _vis:
        vis = oracle.render_terrain(u, W, H, GRID, h, np.zeros(1024, np.uint8), want_vis=True, nthreads=8)[1]
        vis.setflags(write=False)
        _vis[key] = vis
    return _vis[key]


def bases_of(s, settings):
    """the handle's frame without overlays under each setting (before any layer is added)"""
    out = {}
    for name, kw in settings.items():
        s.set_haze(**kw)
        out[name] = s.render_rgba().copy()
    return out


def check_settings(s, bases, settings, vis, u, h, L, what):
    """every setting in turn on the one handle -- no layer is touched in between -- against the model"""
    frames = {}
    for name, kw in settings.items():
        s.set_haze(**kw)
        got = s.render_rgba().copy()
        want = ohm.composite(bases[name], vis, u, h, GRID, L, haze=kw)
        assert_frame(got, want, f"{what} {name}")
        if not frames:
            assert (want != ocm.composite(bases[name], vis, u, h, GRID, L)).any(), f"{what} {name}: the haze changes no overlay pixel"
        frames[name] = got
    return frames


@pytest.mark.parametrize("size", sc.SIZES)
@pytest.mark.parametrize("cam", sc.CAMS)
def test_points_and_polylines_equal_the_model(vf, cam, size):
    import oracle
    W, H = size
    h = heights()
    for precision in ("exact", "fast") if size == sc.SIZES[0] else ("exact",):
        s = scene(vf, W, H, h, cam, precision)
        u = s.debug_uniforms_f32()
        assert np.array_equal(u, oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam]))     # (what the model test's conditions were held on)
        settings = sc.settings(cam) if precision == "exact" else {k: v for k, v in sc.settings(cam).items() if k in ("falloff 0.3", "capped")}
        bases = bases_of(s, settings)
        L = apply(vf, s, sc.layer_calls(cam), ohm.Layers())
        frames = check_settings(s, bases, settings, oracle_vis(u, W, H, h), u, h, L, f"{precision} {cam} {size}")
        names = list(frames)
        assert (frames[names[0]] != frames[names[1]]).any()                                            # new parameters, the same layers: another frame


@pytest.mark.parametrize("cam", sc.CAMS)
def test_a_contour_layer(vf, cam):
    W, H = sc.SIZES[1]
    h = heights()
    s = scene(vf, W, H, h, cam, "exact")
    u = s.debug_uniforms_f32()
    settings = sc.settings(cam)
    bases = bases_of(s, settings)
    levels = np.array([-0.45, 0.65], F32)                        # (near both ends of the surface's heights: the noisy field gives 7 * 10^4 segments there, 10^6 in between)
    kw = dict(width_px=2.0, rgba=(20, 20, 20, 220), lift=0.01, join="round")
    layer = s.add_contours(levels, haze=True, **kw)
    assert s.layer_haze(layer) is True
    L = ohm.Layers().contours(h, GRID, u, levels, haze=True, **kw)
    check_settings(s, bases, settings, oracle_vis(u, W, H, h), u, h, L, f"contours {cam}")


def mixed_calls(occlude=()):
    """hazed and unhazed point / line layers interleaved in layer order over a polygon layer; occlude: the layers (by position) that occlude"""
    rng = np.random.default_rng(31)
    pts = [np.column_stack([rng.uniform(-1.4, 1.4, 150), np.full(150, 0.03), rng.uniform(-1.4, 1.4, 150)]).astype(F32) for _ in range(3)]
    paths = [(rng.uniform(-1.3, 1.3, 3) * [1, 0.02, 1] + [0, 0.03, 0] + np.cumsum(rng.normal(0, 0.3, (4, 3)) * [1, 0.02, 1], axis=0)).astype(F32) for _ in range(25)]
    calls = [("add_polygons", (TRIANGLE,), dict(fill_rgba=(0, 90, 255, 150), line_rgba=(0, 0, 0, 255), line_width_px=2.0, drape=True)),
             ("add_points", (pts[0],), dict(size_px=7.0, rgba=(255, 40, 40, 200), drape=True, haze=True)),
             ("add_points", (pts[1],), dict(size_px=7.0, rgba=(40, 255, 40, 200), shape="square", drape=True)),
             ("add_lines", (paths,), dict(width_px=3.0, rgba=(250, 250, 30, 230), cap="round", drape=True, haze=True)),
             ("add_polygons", (TRIANGLE,), dict(fill_rgba=(200, 0, 200, 90), drape=True)),
             ("add_lines", (paths[::-1],), dict(width_px=1.0, rgba=(0, 0, 0, 255), cap="butt", drape=False)),
             ("add_points", (pts[2],), dict(size_px=4.0, rgba=(255, 255, 255, 255), drape=True, haze=True))]
    return [(m, a, dict(kw, occlude=True, depth_bias=0.02) if k in occlude else kw) for k, (m, a, kw) in enumerate(calls)]


@pytest.mark.parametrize("cam", ["default", "near"])
def test_hazed_and_unhazed_layers_interleaved_over_polygons(vf, cam):
    W, H = sc.SIZES[0]
    h = heights()
    s = scene(vf, W, H, h, cam, "exact")
    u = s.debug_uniforms_f32()
    settings = {k: sc.settings(cam)[k] for k in ("falloff 4.0", "alpha 128")}
    bases = bases_of(s, settings)
    L = apply(vf, s, mixed_calls(), ohm.Layers())
    assert [s.layer_haze(k) for k in range(7)] == [False, True, False, True, False, False, True]
    check_settings(s, bases, settings, oracle_vis(u, W, H, h), u, h, L, f"mixed {cam}")


@pytest.mark.parametrize("occlude", [(1, 3), (2, 5)], ids=["hazed and occluding", "beside an occluding layer"])
@pytest.mark.parametrize("cam", ["default", "near"])
def test_hazed_layers_with_occlusion(vf, cam, occlude):
    W, H = sc.SIZES[0]
    h = heights()
    s = scene(vf, W, H, h, cam, "exact")
    u = s.debug_uniforms_f32()
    vis = oracle_vis(u, W, H, h)
    settings = {k: sc.settings(cam)[k] for k in ("uniform", "falloff 0.3")}
    bases = bases_of(s, settings)
    L = apply(vf, s, mixed_calls(occlude), ohm.Layers())
    frames = check_settings(s, bases, settings, vis, u, h, L, f"occlusion {occlude} {cam}")
    free = ohm.composite(bases["uniform"], np.zeros_like(vis), u, h, GRID, L, haze=settings["uniform"])
    assert (frames["uniform"] != free).any()                     # (the terrain hides something)


def test_more_primitives_in_one_bin_than_a_sort_window_holds(vf):
    W, H = sc.SIZES[0]
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    u = s.debug_uniforms_f32()
    kw = dict(density=0.2, start=1.0, falloff=4.0, base=0.2)
    bases = bases_of(s, {"it": kw})
    eye = np.array(CAMERAS["default"][0])
    axis = -eye / np.linalg.norm(eye)
    n = 5000
    depth = np.where(np.arange(n) % 2 == 0, 2.0, 6.0)            # two alternating depths on the axis: all in one pixel's reach, one bin
    xyz = (eye + depth[:, None] * axis + np.random.default_rng(2).normal(0, 0.004, (n, 3))).astype(F32)
    cols = np.column_stack([np.arange(n) % 256, (np.arange(n) // 7) % 256, np.full(n, 60), np.full(n, 24)]).astype(np.uint8)
    L = apply(vf, s, [("add_points", (xyz,), dict(size_px=1.0, rgba=cols, haze=True))], ohm.Layers())
    check_settings(s, bases, {"it": kw}, oracle_vis(u, W, H, h), u, h, L, "5000 points in one bin")


@pytest.mark.parametrize("size,cam", [((1, 1), "fill"), ((130, 3), "default")])
def test_frames_of_one_pixel_and_of_three_rows(vf, size, cam):
    W, H = size
    h = heights()
    s = scene(vf, W, H, h, cam, "exact")
    u = s.debug_uniforms_f32()
    settings = {k: sc.settings(cam)[k] for k in ("uniform", "falloff 0.3")}
    bases = bases_of(s, settings)
    # (a free point under the grid's centre: deeper than either camera's `start`)
    L = apply(vf, s, [("add_points", (np.array([[0.0, -1.0, 0.0]], F32),), dict(size_px=6.0, rgba=(255, 30, 30, 255), haze=True))], ohm.Layers())
    check_settings(s, bases, settings, oracle_vis(u, W, H, h), u, h, L, f"{size}")


@pytest.mark.parametrize("f", [2, 3])
def test_supersampled_handles_take_hazed_layers(vf, f):
    W, H = 37, 23
    h = heights()
    s = vf.Scene(W, H, grid=GRID, supersample=f)
    s.set_height_from_r32f(h)
    s.set_camera_look_at(*CAMERAS["default"])
    u = s.debug_uniforms_f32()
    settings = {k: sc.settings("default")[k] for k in ("falloff 4.0", "capped")}
    bases = bases_of(s, settings)
    L = apply(vf, s, sc.layer_calls("default"), ohm.Layers())
    check_settings(s, bases, settings, np.zeros((H, W), np.uint32), u, h, L, f"supersample {f}")


def test_the_flag_goes_off_and_on_and_clear_overlays_starts_over(vf):
    W, H = sc.SIZES[0]
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    u = s.debug_uniforms_f32()
    vis = oracle_vis(u, W, H, h)
    kw = sc.settings("default")["falloff 4.0"]
    base = bases_of(s, {"it": kw})["it"]
    calls = sc.line_calls()[:2] + sc.point_calls()[:2]
    L = apply(vf, s, calls, ohm.Layers())
    hazed = s.render_rgba().copy()
    assert_frame(hazed, ohm.composite(base, vis, u, h, GRID, L, haze=kw), "all hazed")
    plain = ocm.composite(base, vis, u, h, GRID, L)
    for k in range(4):
        assert s.layer_haze(k) is True
        s.set_layer_haze(k, False)
        L.set_haze(k, False)
        assert s.layer_haze(k) is False
        assert_frame(s.render_rgba(), ohm.composite(base, vis, u, h, GRID, L, haze=kw), f"layer {k} off")
    assert_frame(s.render_rgba(), plain, "every flag off: the unhazed bytes")
    for k in range(4):
        s.set_layer_haze(k)                                        # (on is the default)
    assert_frame(s.render_rgba(), hazed, "on again: the hazed bytes")
    s.clear_overlays()
    assert_frame(s.render_rgba(), base, "no overlays")
    layer = s.add_points(calls[2][1][0], **dict(calls[2][2], haze=False))
    assert layer == 0 and s.layer_haze(0) is False               # the ids start over, unflagged
    P = ohm.Layers().points(calls[2][1][0], **dict(calls[2][2], haze=False))
    assert_frame(s.render_rgba(), ocm.composite(base, vis, u, h, GRID, P), "after clear_overlays")
    t = vf.TerrainSpike(160, 120, grid=48)                        # the other class
    k = t.add_points(np.zeros((1, 3), F32), size_px=9.0, haze=True)
    assert t.layer_haze(k) is True
    t.set_layer_haze(k, False)
    assert t.layer_haze(k) is False


def test_haze_off_gives_the_bytes_of_the_same_layers_unflagged(vf):
    W, H = sc.SIZES[1]
    h = heights()
    kw = sc.settings("fill")["falloff 0.3"]
    calls = sc.layer_calls("fill")
    flagged, unflagged = scene(vf, W, H, h, "fill", "exact"), scene(vf, W, H, h, "fill", "exact")
    for m, a, k in calls:
        getattr(flagged, m)(*a, **k)
        getattr(unflagged, m)(*a, **dict(k, haze=False))
    never = flagged.render_rgba().copy()                           # haze never set
    assert np.array_equal(never, unflagged.render_rgba())
    flagged.set_haze(**kw)
    unflagged.set_haze(**kw)
    on = flagged.render_rgba().copy()
    assert (on != unflagged.render_rgba()).any()
    for off in (dict(kw, enabled=False), dict(kw, density=0.0)):
        flagged.set_haze(**off)
        unflagged.set_haze(**off)
        assert np.array_equal(flagged.render_rgba(), unflagged.render_rgba()), off
    assert np.array_equal(flagged.render_rgba(), never)            # (density 0 hazes no terrain either)
    flagged.set_haze(**kw)
    assert np.array_equal(flagged.render_rgba(), on)
    flagged.clear_haze()
    assert np.array_equal(flagged.render_rgba(), never)            # cleared
    assert flagged.layer_haze(0) is True                           # (the flag rests with the layer)


def test_a_height_upload_moves_a_draped_hazed_layer(vf):
    W, H = sc.SIZES[0]
    h, h2 = heights(), heights(9) * F32(2.5)
    cam = "default"
    kw = sc.settings(cam)["falloff 0.3"]                          # (the height matters most under a shallow layer of haze)
    s = scene(vf, W, H, h, cam, "exact")
    u = s.debug_uniforms_f32()
    base = bases_of(s, {"it": kw})["it"]
    calls = [c for c in sc.layer_calls(cam) if c[2]["drape"]]
    L = apply(vf, s, calls, ohm.Layers())
    first = s.render_rgba().copy()
    assert_frame(first, ohm.composite(base, oracle_vis(u, W, H, h), u, h, GRID, L, haze=kw), "first heights")
    s.set_height_from_r32f(h2)
    s2 = scene(vf, W, H, h2, cam, "exact")
    s2.set_haze(**kw)
    base2 = s2.render_rgba().copy()
    got = s.render_rgba().copy()
    assert_frame(got, ohm.composite(base2, oracle_vis(u, W, H, h2), u, h2, GRID, L, haze=kw), "second heights")
    assert (got != first).any()


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    W, H = sc.SIZES[0]
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    s.set_haze(**sc.settings("default")["uniform"])
    s.add_points(np.array([[0.3, 0.05, 0.2]], F32), size_px=9.0, drape=True, haze=True)
    s.add_polygons(TRIANGLE, fill_rgba=(0, 90, 255, 150), line_rgba=(0, 0, 0, 255))
    want = s.render_rgba().copy()
    with pytest.raises(RuntimeError, match="a polygon layer cannot take the haze: polygon fills have no depth"):
        s.set_layer_haze(1, True)
    with pytest.raises(RuntimeError, match="no overlay layer with that id"):
        s.set_layer_haze(2, True)
    with pytest.raises(RuntimeError, match="no overlay layer with that id"):
        s.layer_haze(2)
    with pytest.raises(TypeError, match="haze must be a bool"):
        s.add_points(np.zeros((1, 3), F32), haze=1)
    with pytest.raises(TypeError, match="on must be a bool"):
        s.set_layer_haze(0, "yes")
    assert s.layer_haze(0) is True and s.layer_haze(1) is False
    assert np.array_equal(s.render_rgba(), want)                  # the next frame is unchanged
    with pytest.raises(RuntimeError, match="render_batch on a handle with haze enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])     # (the haze's own rule)
    assert np.array_equal(s.render_rgba(), want)
    t = cabi.Terrain(64, 128, 32, np.zeros(1024, np.uint8))
    t.add_points(np.zeros((2, 3), F32))
    assert t.layer_haze(0) is False
    assert t.lib.vf_terrain_set_layer_haze(t.t, 5, 1) == cabi.VF_ERR_INVALID
    t.set_layer_haze(0)
    assert t.layer_haze(0) is True
    t.close()
