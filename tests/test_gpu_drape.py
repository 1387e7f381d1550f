"""The draped image layer on the GPU equals the CPU model (tests/drape_model) bit for bit: three cameras, two sizes, both
shade modes, both precisions, both filters, RGB and RGBA, image sizes from one texel to the limit strips, full, interior and
overhanging extents, two opacities, with cast shadows and ambient occlusion, under overlays, after one image replaces another;
and nothing else moves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import drape_model as drm
import occlusion_model as ocm
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from support import bits, vf, viridis  # noqa: F401

abm, shm = drm.abm, drm.shm
SIZES = [(257, 131), (640, 363)]                              # neither width is a multiple of 32, neither height one of 8
EXTENTS = {"full": None, "interior": (-0.7, -0.5, 0.9, 0.8), "overhanging": drm.EXTENT}


def model(u, W, H, h, mode, img, **kw):
    rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
    frame, again = drm.frame(rgba, vis, u, h, GRID, viridis(), img, shade_mode=1 if mode == "spec_t32" else 0, **kw)
    return frame, again, vis


def assert_frame(got, want, what, where=None):
    # byte for byte, at the pixels of the mask `where` if one is given
    support.assert_frame(got if where is None else np.where(where[..., None], got, want), want, what)


def assert_draped(s, plain, precision, want, what):
    """the scene's frame against the model's (frame, rewritten, vis): in `fast` the pixels that are not written again keep `plain`'s bytes"""
    frame, again, _ = want
    got = s.render_rgba().copy()
    if precision == "exact":
        assert_frame(got, frame, what)
    else:
        assert_frame(got, frame, what + ", rewritten pixels", again)
        assert_frame(got, plain, what + ", other pixels", ~again)
    return got


@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, size, mode):
    W, H = size
    h = heights()
    rgb = drm.image()[..., :3].copy()
    cases = [(drm.image(), dict(extent=drm.SCENE_EXTENT[cam], opacity=1.0, filter="linear")),
             (drm.image(), dict(extent=drm.SCENE_EXTENT[cam], opacity=0.37, filter="nearest")),
             (rgb, dict(extent=drm.SCENE_EXTENT[cam], opacity=0.37, filter="linear")),
             (rgb, dict(extent=drm.SCENE_EXTENT[cam], opacity=1.0, filter="nearest"))]
    want = {}
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        plain = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
        for k, (img, kw) in enumerate(cases):
            s.set_drape(img, **kw)
            if k not in want:
                want[k] = model(u, W, H, h, mode, img, **kw)
                frame, again, vis = want[k]
                frac = again.sum() / max(int((vis != 0).sum()), 1)
                print(f"{cam} {W}x{H} {mode} case {k}: {frac:.3f} of the covered pixels are written again")
                assert 0.1 <= frac <= 0.9
            got = assert_draped(s, plain, precision, want[k], f"{precision} {cam} {size} {mode} case {k}")
            assert (got != plain).any()
            assert np.array_equal(s.render_rgba(), got)
        s.clear_drape()
        assert np.array_equal(s.render_rgba(), plain) and s.drape_info() is None


@pytest.mark.parametrize("isize", [(1, 1), (2, 3), (37, 53), (16384, 2), (2, 16384)])
def test_image_sizes_and_extents(vf, isize):
    W, H = 257, 131
    h = heights()
    img = drm.image(size=isize)
    if not img[..., 3].any():                                 # (smaller than the pattern's first hole)
        img[..., 3] = np.random.default_rng(2).integers(1, 256, img.shape[:2], dtype=np.uint8)
    for cam in ("fill", "near"):
        s = scene(vf, W, H, h, cam, "exact")
        u = s.debug_uniforms_f32()
        plain = s.render_rgba().copy()
        for name, ext in EXTENTS.items():
            for filt in ("linear", "nearest"):
                s.set_drape(img, extent=ext, filter=filt)
                want = model(u, W, H, h, "reference", img, extent=ext, filter=filt)
                assert want[1].any()
                assert_draped(s, plain, "exact", want, f"{isize} {cam} {name} {filt}")
                info = s.drape_info()
                assert (info["width"], info["height"], info["filter"], info["opacity"]) == (isize[0], isize[1], filt, 1.0)
                assert info["extent"] == tuple(float(np.float32(v)) for v in (drm.FULL_EXTENT if ext is None else ext))


@pytest.mark.parametrize("features", ["shadows", "ambient", "both"])
@pytest.mark.parametrize("cam,mode", [("default", "reference"), ("fill", "reference"), ("near", "reference"), ("default", "spec_t32")])
def test_with_shadows_and_ambient_occlusion(vf, cam, mode, features):
    W, H = 257, 131
    h = abm.scene_heights()
    shadows, ambient = features != "ambient", features != "shadows"
    strength = abm.SCENE_PARAMS["strength"]
    kw = dict(extent=drm.SCENE_EXTENT[cam], opacity=0.37, filter="linear")
    want = None
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        s.set_sun(*abm.SCENE_SUN_DEG)
        s.set_shadows(shadows, **abm.SCENE_SHADOWS)
        s.set_ambient_occlusion(ambient, strength=strength, reach=abm.SCENE_PARAMS["reach"], directions=abm.scene_directions())
        before = s.render_rgba().copy()                       # shadowed / occluded, not draped
        u = s.debug_uniforms_f32()
        s.set_drape(drm.image(), **kw)
        if want is None:
            lit = shm.field(u, h, GRID, **abm.SCENE_SHADOWS) if shadows else None
            sky = abm.field(u, h, GRID, abm.scene_directions(), abm.SCENE_PARAMS["reach"]) if ambient else None
            rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
            # the drape goes over the frame the shadow / ambient pass left: its model first
            base, _ = abm.frame(rgba, vis, u, h, GRID, viridis(), sky if ambient else np.ones((GRID, GRID), np.float32), strength, lit=lit,
                                shade_mode=1 if mode == "spec_t32" else 0)
            frame, again = drm.frame(base, vis, u, h, GRID, viridis(), drm.image(), lit=lit, sky=sky, strength=strength,
                                     shade_mode=1 if mode == "spec_t32" else 0, **kw)
            assert again.any() and (base != rgba).any() and (frame != base).any()
            want = (frame, again, vis)
        assert_draped(s, before, precision, want, f"{precision} {cam} {mode} {features}")
        s.clear_drape()
        assert np.array_equal(s.render_rgba(), before)


def overlay_calls(seed=5):
    rng = np.random.default_rng(seed)
    n = 600
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-0.05, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.08, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(60)]
    poly = [np.array([[-0.6, 0.05, -0.6], [0.7, 0.05, -0.5], [0.1, 0.05, 0.8]], np.float32)]
    return [("add_points", (pts,), dict(size_px=5.0, rgba=(255, 0, 0, 200), drape=True, occlude=True)),
            ("add_lines", (paths,), dict(width_px=3.0, rgba=(0, 255, 0, 200), drape=False)),
            ("add_lines", (paths[:30],), dict(width_px=2.0, rgba=(255, 255, 0, 255), drape=False, occlude=True, depth_bias=1e-3)),
            ("add_polygons", (poly,), dict(fill_rgba=(0, 90, 255, 160), line_rgba=(0, 0, 0, 255), line_width_px=2.0, drape=True))]


def test_overlays_composite_over_the_draped_frame(vf):
    W, H = 257, 131
    h = heights()
    kw = dict(extent=drm.EXTENT, opacity=1.0, filter="linear")
    for cam in ("default", "near"):
        s = scene(vf, W, H, h, cam, "exact")
        u = s.debug_uniforms_f32()
        s.set_drape(drm.image(), **kw)
        L = apply(vf, s, overlay_calls(), ocm.Layers())
        base, again, vis = model(u, W, H, h, "reference", drm.image(), **kw)
        want = ocm.composite(base, vis, u, h, GRID, L)
        assert again.any() and (want != base).any() and not np.array_equal(want, ocm.pm.composite(base, u, h, GRID, L))
        assert_frame(s.render_rgba(), want, f"overlays over the drape, {cam}")


def test_one_image_replaces_another(vf):
    W, H = 257, 131
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    u = s.debug_uniforms_f32()
    plain = s.render_rgba().copy()
    big, small = drm.opaque_image((301, 77)), drm.image()
    for img, kw in ((big, dict(extent=None, filter="nearest")), (small, dict(extent=drm.EXTENT, opacity=0.37)), (big[:9, :5, :3].copy(), dict(filter="linear")),
                    (big, dict(extent=(-3.0, -3.0, 0.2, 0.1), filter="linear"))):
        s.set_drape(img, **kw)
        assert_draped(s, plain, "exact", model(u, W, H, h, "reference", img, **kw), f"replaced by {img.shape}")
    snapshot = small.copy()
    s.set_drape(snapshot, extent=drm.EXTENT)
    snapshot[:] = 0                                           # the handle holds a copy made at the call
    assert_draped(s, plain, "exact", model(u, W, H, h, "reference", small, extent=drm.EXTENT), "a snapshot")


def test_nothing_else_moves(vf):
    W, H = 257, 131
    h = heights(5)
    never = scene(vf, W, H, h, "near")
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    vis = never.debug_visibility().copy()
    s = scene(vf, W, H, h, "near")
    assert s.drape_info() is None
    s.clear_drape()                                           # (nothing to clear)
    s.set_drape(drm.image(), extent=drm.EXTENT, opacity=0.37, filter="nearest")
    info = s.drape_info()
    assert info == {"width": 37, "height": 53, "extent": tuple(float(np.float32(v)) for v in drm.EXTENT), "opacity": float(np.float32(0.37)),
                    "filter": "nearest"}
    draped = s.render_rgba().copy()
    assert (draped != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), vis)
    assert np.array_equal(s.render_rgba(), draped)
    s.clear_drape()
    assert s.drape_info() is None and np.array_equal(s.render_rgba(), want)
    sp = vf.TerrainSpike(160, 120, grid=48)
    spike = sp.render_rgba().copy()
    sp.set_drape(drm.opaque_image((8, 8)))
    assert sp.drape_info()["width"] == 8 and (sp.render_rgba() != spike).any()
    sp.clear_drape()
    assert np.array_equal(sp.render_rgba(), spike)


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    W, H = 128, 128
    h = heights(2, (32, 32))
    img = drm.image()
    s = scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_drape(img)
    s.set_shard(0, 1, 64)
    assert s.drape_info() is None
    u = support.uniforms(W, H)
    t = cabi.Terrain(W, H, 32, viridis())
    t.set_height(h)
    t.set_uniforms(u)
    t.set_tile_shard(0, 2)
    ext = (cabi.C.c_float * 4)(-1.5, -1.5, 1.5, 1.5)
    assert t.lib.vf_terrain_set_drape(t.t, img.ctypes.data, 37, 53, 4, ext, 1.0, 1) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode() and t.drape_info() is None
    t.close()
    t = cabi.Terrain(W, H, 32, viridis())
    t.set_height(h)
    t.set_uniforms(u)
    t.set_drape(img, extent=drm.EXTENT, opacity=0.37, filter="nearest")
    info = t.drape_info()
    t.render()
    draped = t.read_rgba().copy()
    nan, inf = float("nan"), float("inf")
    E = lambda *v: (cabi.C.c_float * 4)(*v)
    p = img.ctypes.data
    for bad in ((p, 0, 53, 4, ext, 1.0, 1), (p, 37, 0, 4, ext, 1.0, 1), (p, 16385, 1, 4, ext, 1.0, 1), (p, 1, 16385, 4, ext, 1.0, 1),
                (p, 37, 53, 2, ext, 1.0, 1), (p, 37, 53, 5, ext, 1.0, 1), (None, 37, 53, 4, ext, 1.0, 1),
                (p, 37, 53, 4, E(0, 0, 0, 1), 1.0, 1), (p, 37, 53, 4, E(0, 1, 1, 1), 1.0, 1), (p, 37, 53, 4, E(1, 0, 0, 1), 1.0, 1),
                (p, 37, 53, 4, E(nan, 0, 1, 1), 1.0, 1), (p, 37, 53, 4, E(0, 0, inf, 1), 1.0, 1),
                (p, 37, 53, 4, ext, 1.5, 1), (p, 37, 53, 4, ext, -0.1, 1), (p, 37, 53, 4, ext, nan, 1), (p, 37, 53, 4, ext, 1.0, 2), (p, 37, 53, 4, ext, 1.0, -1)):
        assert t.lib.vf_terrain_set_drape(t.t, *bad) == cabi.VF_ERR_INVALID, bad[1:]
        assert t.drape_info() == info
    assert t.lib.vf_terrain_set_drape_device(t.t, None, 37, 53, ext, 1.0, 1, None) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_set_shard(t.t, 0, 2, 64) == cabi.VF_ERR_INVALID and "draped image" in t.lib.vf_last_error().decode()
    assert t.lib.vf_terrain_set_tile_shard(t.t, 0, 2, 3) == cabi.VF_ERR_INVALID and "draped image" in t.lib.vf_last_error().decode()
    with pytest.raises(RuntimeError, match="render_batch on a handle that holds a draped image"):
        t.render_batch(np.stack([u, u]))
    t.render()
    assert np.array_equal(t.read_rgba(), draped) and t.drape_info() == info
    assert t.drape_stage(2) > 0 and t.drape_info() == info
    t.close()
    s.set_drape(img)
    with pytest.raises(RuntimeError, match="render_batch on a handle that holds a draped image"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="draped image"):
        s.set_shard(0, 2, 64)
    with pytest.raises(ValueError, match="opacity"):
        s.set_drape(img, opacity=2.0)
    with pytest.raises(TypeError, match="image must be"):
        s.set_drape(img.astype(np.float32))
    assert s.drape_info()["opacity"] == 1.0


def test_the_stage_calls_hand_the_scan_counters_back():
    """drape_stage brings the shadow and sky-view fields up to date itself, ambient_stage the shadow field: diagnostic launches are
    not the handle's, whichever call makes them"""
    from vulkan_forge_amd import cabi
    W, H = 257, 131
    u = support.uniforms(W, H)
    u[32:35] = shm.sun_vector(*abm.SCENE_SUN_DEG)
    t = cabi.Terrain(W, H, 32, viridis())
    t.set_height(heights(2, (32, 32)))
    t.set_uniforms(u)
    t.set_shadows(True, **abm.SCENE_SHADOWS)
    t.set_ambient_occlusion(True, strength=abm.SCENE_PARAMS["strength"], reach=abm.SCENE_PARAMS["reach"], directions=abm.scene_directions())
    t.set_drape(drm.image(), extent=drm.EXTENT, opacity=0.37, filter="linear")
    t.render()
    frame = t.read_rgba().copy()
    info, scans = t.drape_info(), (t.shadow_scans(), t.ambient_scans())
    assert scans == (1, 1) and info["width"] == 37 and info["height"] == 53
    ms = (t.drape_stage(2), *t.ambient_stage(2), *t.shadow_stage(2))
    print("drape, ambient field, ambient shade, shadow field, shadow shade ms:", ms)
    assert all(v > 0 for v in ms)
    assert (t.shadow_scans(), t.ambient_scans()) == scans
    t.render()
    assert np.array_equal(t.read_rgba(), frame) and t.drape_info() == info
    assert (t.shadow_scans(), t.ambient_scans()) == scans
    t.close()


def test_the_image_from_device_memory_on_a_stream_of_the_callers():
    support.run_check("drape_torch_check.py", "DRAPE TORCH OK")
