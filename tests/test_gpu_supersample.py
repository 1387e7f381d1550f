"""Supersampled terrain frames on the GPU against the CPU model (tests/supersample_model), bit for bit in exact
precision: the samples equal the oracle's frame at (f W, f H), the frame equals the model's resolve of them, the overlays composite
at the output size; at sizes chosen for the resolve's edges -- 71 x 45 (odd; neither W nor f W a multiple of the 64-pixel tile;
f = 3 rows not 16-byte aligned), 64 x 64 (exact tiles), 1 x 1, 130 x 3 (wider than one wave's row segment, shorter than a tile) --
for f = 2, 3, 4; with every pass and every kind of overlay at once; geometry buffers and pick; the read-backs; every kind of change;
the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import supersample_model as ssm
from support import vf, viridis  # noqa: F401

F32 = np.float32
GRID = 33
SIZES = [(71, 45), (64, 64), (1, 1), (130, 3)]
FACTORS = [2, 3, 4]
CAMERAS = {
    "default": ((3.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0),
    "grazing": ((0.0, 0.5, 3.2), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), 42.0, 0.1, 100.0),
}


def heights(seed=11, shape=(33, 33)):
    return (np.random.default_rng(seed).random(shape, dtype=F32) * 0.6 - 0.3).astype(F32)


def scene(vf, W, H, f, h, cam="default", precision="exact", grid=GRID):
    s = vf.Scene(W, H, grid=grid, supersample=f)
    s.set_height_from_r32f(h)
    s.set_shade_precision(precision)
    s.set_camera_look_at(*CAMERAS[cam])
    return s


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    d = got != want
    d = d.any(axis=2) if d.ndim == 3 else d
    assert not d.any(), f"{what}: {int(d.sum())} pixels differ, first at {np.argwhere(d)[:4].tolist()}"


def lsb(a, b):
    return int(np.abs(a.astype(np.int16) - b.astype(np.int16)).max())


_models = {}


def model(W, H, f, cam, h, u):
    """the model of the plain frame (computed once per case, and left unchanged)"""
    key = (W, H, f, cam, support.digest(h), u.tobytes())
    if key not in _models:
        _models[key] = support.frozen(ssm.frame(W, H, f, u, h, GRID, viridis()))
    return _models[key]


# ---- 1. the samples, the visibility and the frame, in both precisions ----

@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("f", FACTORS)
@pytest.mark.parametrize("size", SIZES)
def test_samples_visibility_and_frame_equal_the_model(vf, size, f, cam):
    W, H = size
    h = heights()
    s = scene(vf, W, H, f, h, cam)
    assert (s.supersample, s.samples, s.sample_size) == (f, f * f, (f * W, f * H))
    u = s.debug_uniforms_f32()
    m = model(W, H, f, cam, h, u)
    frame = s.render_rgba().copy()
    samples = s.render_samples()
    assert frame.shape == (H, W, 4) and samples.shape == (f * H, f * W, 4)
    assert_same(samples, m["samples"], "samples against the oracle's frame at the sample size")
    assert_same(s.debug_visibility(), m["vis"], "visibility")
    assert_same(frame, ssm.resolve(samples, f), "frame against the model's resolve of the samples")
    assert_same(frame, m["frame"], "frame against the model")
    if min(W, H) > 3:
        assert (m["vis"] != 0).any() and (m["vis"] == 0).any()            # (terrain and background both show)
    s.set_shade_precision("fast")
    fast = s.render_rgba().copy()
    fast_samples = s.render_samples()
    assert lsb(fast_samples, m["samples"]) <= 1 and lsb(fast, m["frame"]) <= 1
    assert_same(fast, ssm.resolve(fast_samples, f), "fast frame against the model's resolve of its own samples")


# ---- 2. factor 1 through the new entry point is vf_terrain_create's handle ----

def test_factor_one_is_the_plain_handle():
    import oracle
    from vulkan_forge_amd import cabi
    W, H = 71, 45
    h = heights()
    u = oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"])
    got = []
    for ss in (None, 1):
        t = cabi.Terrain(W, H, GRID, viridis(), supersample=ss)
        t.set_height(h)
        t.set_uniforms(u)
        t.render()
        assert t.supersampling() == (1, W, H)
        got.append((t.read_rgba(), t.read_visibility(), t.read_png_scanlines()))
        with pytest.raises(cabi.VfError, match="not supersampled"):
            t.read_samples()
        t.close()
    for a, b, what in zip(got[0], got[1], ("frame", "visibility", "png scanlines")):
        assert_same(b, a, what)
    assert (got[0][1] != 0).any()


# ---- 3. everything at once ----

def everything():
    rng = np.random.default_rng(21)
    feats = dict(
        shadows=dict(strength=0.8, softness=0.05, bias=0.01),
        ambient=dict(directions=np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], F32), reach=8.0, strength=0.6),
        drape=dict(image=rng.integers(0, 256, (29, 37, 4), dtype=np.uint8), extent=(-1.2, -1.0, 1.1, 1.3), opacity=0.8, filter="linear", mips=True, bias=0.0),
        viewshed=dict(observer=(0.4, 0.3), eye_height=1.0, target_height=0.0, softness=0.1, bias=0.01, visible_rgba=(64, 255, 96, 96), hidden_rgba=(200, 0, 0, 90)),
        cumulative=dict(observers=rng.uniform(-1.3, 1.3, (3, 2)).astype(F32), eye_height=0.6, target_height=0.02, softness=0.05, bias=0.01,
                        high_rgba=(64, 255, 96, 120), low_rgba=(90, 0, 0, 60)),
        exposure=dict(suns=np.array([(0.5, 1.0, 0.3), (-0.6, 0.4, 0.2), (0.1, 0.7, -0.9)], F32), weights=np.array([1.0, 0.5, 0.8], F32), incidence=False,
                      softness=0.1, bias=0.05, high_rgba=(255, 208, 64, 160), low_rgba=(0, 60, 255, 100)))
    pts = np.column_stack([rng.uniform(-1.4, 1.4, 40), rng.uniform(0.0, 0.3, 40), rng.uniform(-1.4, 1.4, 40)]).astype(F32)
    paths = [(rng.uniform(-1.2, 1.2, 3) * [1, 0.1, 1] + np.cumsum(rng.normal(0, 0.2, (4, 3)) * [1, 0.1, 1], axis=0)).astype(F32) for _ in range(6)]
    outer = np.array([(-1.0, 0.2, -1.0), (1.0, 0.2, -0.9), (0.9, 0.2, 1.0), (-0.8, 0.2, 0.8)], F32)
    hole = np.array([(-0.3, 0.2, -0.3), (0.3, 0.2, -0.3), (0.3, 0.2, 0.3), (-0.3, 0.2, 0.3)], F32)
    overlays = dict(points=dict(xyz=pts, size_px=5.0, rgba=(255, 0, 0, 150), shape="circle", drape=True),
                    lines=dict(paths=paths, width_px=2.5, rgba=(255, 255, 0, 120), cap="round", drape=False),
                    polygons=dict(polygons=[[outer, hole]], fill_rgba=(0, 90, 255, 110), line_rgba=(255, 255, 255, 140), line_width_px=1.5, drape=True),
                    contours=dict(levels=np.array([-0.15, 0.0, 0.15], F32), width_px=1.0, rgba=(0, 0, 0, 130), lift=0.0, join="round"))
    return feats, overlays


def apply_everything(s, feats, overlays):
    s.set_shadows(True, **feats["shadows"])
    a = feats["ambient"]
    s.set_ambient_occlusion(True, strength=a["strength"], reach=a["reach"], directions=a["directions"])
    d = feats["drape"]
    s.set_drape(d["image"], extent=d["extent"], opacity=d["opacity"], filter=d["filter"])
    s.set_drape_mipmaps(True, bias=d["bias"])
    v = dict(feats["viewshed"])
    s.set_viewshed(v.pop("observer"), **v)
    c = dict(feats["cumulative"])
    s.set_cumulative_viewshed(c.pop("observers"), **c)
    e = dict(feats["exposure"])
    s.set_sun_exposure(e.pop("suns"), **e)
    o = overlays
    s.add_points(o["points"]["xyz"], **{k: w for k, w in o["points"].items() if k != "xyz"})
    s.add_lines(o["lines"]["paths"], **{k: w for k, w in o["lines"].items() if k != "paths"})
    s.add_polygons(o["polygons"]["polygons"], **{k: w for k, w in o["polygons"].items() if k != "polygons"})
    s.add_contours(o["contours"]["levels"], **{k: w for k, w in o["contours"].items() if k != "levels"})


def model_layers(overlays, h, u):
    import contour_model as cm
    L = cm.Layers()
    o = overlays
    L.points(o["points"]["xyz"], **{k: w for k, w in o["points"].items() if k != "xyz"})
    L.lines(o["lines"]["paths"], **{k: w for k, w in o["lines"].items() if k != "paths"})
    L.polygons(o["polygons"]["polygons"], **{k: w for k, w in o["polygons"].items() if k != "polygons"})
    L.contours(h, GRID, u, o["contours"]["levels"], **{k: w for k, w in o["contours"].items() if k != "levels"})
    return L


@pytest.mark.parametrize("f", [2, 3])
def test_every_pass_and_every_kind_of_overlay_at_once(vf, f):
    W, H = 71, 45
    h = heights()
    feats, overlays = everything()
    s = scene(vf, W, H, f, h)
    apply_everything(s, feats, overlays)
    u = s.debug_uniforms_f32()
    m = ssm.frame(W, H, f, u, h, GRID, viridis(), layers=model_layers(overlays, h, u), **feats)
    plain = model(W, H, f, "default", h, u)
    frame = s.render_rgba().copy()
    samples = s.render_samples()
    assert (m["samples"] != plain["samples"]).any() and (m["frame"] != m["resolved"]).any()      # (the passes and the overlays both show)
    assert_same(samples, m["samples"], "samples against the composed feature models at the sample size")
    assert_same(frame, m["frame"], "frame against the model")
    assert_same(s.render_rgba(), frame, "a second render")


# ---- 4. geometry buffers and pick ----

@pytest.mark.parametrize("f", FACTORS)
def test_gbuffer_planes_are_the_samples_and_pick_answers_for_the_representative(vf, f):
    import gbuffer_model as gbm
    W, H = 71, 45
    h = heights()
    s = scene(vf, W, H, f, h, "grazing")
    u = s.debug_uniforms_f32()
    vis = model(W, H, f, "grazing", h, u)["vis"]
    g = s.render_gbuffer()
    depth, position, normal = gbm.planes(vis, u, h, GRID)
    want = {"depth": depth, "position": position, "normal": normal, "primitive": vis}
    for k in want:
        assert g[k].shape == want[k].shape == (f * H, f * W) + want[k].shape[2:]
        assert np.array_equal(np.ascontiguousarray(g[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), k
    assert np.array_equal(s.render_depth().view(np.uint32), depth.view(np.uint32))
    px = np.concatenate([[(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)],
                         np.column_stack([np.random.default_rng(6).integers(0, W, 16), np.random.default_rng(7).integers(0, H, 16)])]).astype(np.int32)
    got = s.pick(px)
    for k in want:
        rep = ssm.representative(want[k], f)
        assert rep.shape[:2] == (H, W)
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(rep[px[:, 1], px[:, 0]]).view(np.uint32)), k
    assert (got["primitive"] != 0).any()
    with pytest.raises(ValueError, match="outside the 71 x 45 frame"):
        s.pick([[W, 0]])


# ---- 5. the read-backs ----

@pytest.mark.parametrize("f", FACTORS)
def test_render_png_decodes_to_the_frame(vf, f, tmp_path):
    from PIL import Image
    W, H = 71, 45
    s = scene(vf, W, H, f, heights())
    path = str(tmp_path / "frame.png")
    s.render_png(path)
    img = np.asarray(Image.open(path))
    assert img.shape == (H, W, 4)
    assert_same(img, s.render_rgba(), "png")


def test_device_destinations():
    """set_output_device with a torch tensor of W x H x 4 receives the frame and samples_device fills an f W x f H x 4 tensor (a
    fresh process: torch is imported before the library there, one HIP runtime per process)"""
    support.run_check("supersample_torch_check.py", "SUPERSAMPLE TORCH OK")


# ---- 6. change, then render ----

@pytest.mark.parametrize("f", FACTORS)
def test_the_frame_follows_every_kind_of_change(vf, f):
    W, H = 71, 45
    h0, h1 = heights(), heights(12)
    s = scene(vf, W, H, f, h0)
    u0 = s.debug_uniforms_f32()
    first = model(W, H, f, "default", h0, u0)
    assert_same(s.render_rgba(), first["frame"], "first")
    s.set_height_from_r32f(h1)                                   # new heights
    assert_same(s.render_rgba(), ssm.frame(W, H, f, u0, h1, GRID, viridis())["frame"], "new heights")
    s.set_camera_look_at(*CAMERAS["grazing"])                    # a new camera
    u1 = s.debug_uniforms_f32()
    m1 = ssm.frame(W, H, f, u1, h1, GRID, viridis())
    assert_same(s.render_rgba(), m1["frame"], "new camera")
    s.set_shade_precision("fast")                                # exact <-> fast
    assert lsb(s.render_rgba(), m1["frame"]) <= 1
    s.set_shade_precision("exact")
    assert_same(s.render_rgba(), m1["frame"], "exact again")
    sh = dict(strength=0.8, softness=0.05, bias=0.01)
    s.set_shadows(True, **sh)                                    # shadows on then off
    m2 = ssm.frame(W, H, f, u1, h1, GRID, viridis(), shadows=sh)
    assert (m2["frame"] != m1["frame"]).any()
    assert_same(s.render_rgba(), m2["frame"], "shadows on")
    assert_same(s.render_samples(), m2["samples"], "shadowed samples")
    s.set_shadows(False)
    assert_same(s.render_rgba(), m1["frame"], "shadows off")
    import contour_model as cm                                   # a translucent layer, then clear_overlays
    pts = np.array([(0.0, 0.2, 0.0), (0.5, 0.1, -0.4), (-0.7, 0.0, 0.6)], F32)
    s.add_points(pts, size_px=9.0, rgba=(255, 0, 0, 128))
    L = cm.Layers()
    L.points(pts, size_px=9.0, rgba=(255, 0, 0, 128))
    m3 = ssm.composite(m1["resolved"], u1, h1, GRID, L)
    assert (m3 != m1["frame"]).any()
    assert_same(s.render_rgba(), m3, "a translucent layer")
    assert_same(s.render_rgba(), m3, "a translucent layer, rendered again")      # (the overlays never composite twice)
    s.clear_overlays()
    assert_same(s.render_rgba(), m1["frame"], "clear_overlays")
    s.set_height_from_r32f(h0)
    s.set_camera_look_at(*CAMERAS["default"])
    assert_same(s.render_rgba(), first["frame"], "back at the first state")


# ---- 7. the refusals ----

def test_refusals_leave_a_usable_handle(vf):
    import ctypes
    import oracle
    from vulkan_forge_amd import cabi
    W, H, f = 71, 45, 2
    h = heights()
    u = oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"])
    want = model(W, H, f, "default", h, np.asarray(u, F32))["frame"]
    t = cabi.Terrain(W, H, GRID, viridis(), supersample=f)
    t.set_height(h)
    t.set_uniforms(u)
    t.set_shade_precision(0)                                     # exact

    def still_renders(what):
        t.render()
        assert_same(t.read_rgba(), want, what)

    still_renders("before any refusal")
    # the factor and the size limits, through the library itself
    lut = np.ascontiguousarray(viridis(), np.uint8).reshape(1024)
    for args, msg in (((8, 8, 0), "factor 0 is outside 1..4"), ((8, 8, 5), "factor 5 is outside 1..4"),
                      ((4097, 8, 4), "exceed the 16384 x 16384 frame limit"), ((8, 5462, 3), "exceed the 16384 x 16384 frame limit")):
        out = ctypes.c_void_p()
        rc = t.lib.vf_terrain_create_supersampled(t.ctx, args[0], args[1], 8, lut.ctypes.data, 1, args[2], ctypes.byref(out))
        assert rc == cabi.VF_ERR_INVALID and not out.value and msg in t.lib.vf_last_error().decode(), (args, t.lib.vf_last_error())
    still_renders("after refused creations")
    with pytest.raises(cabi.VfError, match="supersampled"):
        t.set_tile_shard(0, 2, 3)
    with pytest.raises(cabi.VfError, match="supersampled"):
        t.set_shard(0, 2, 64)
    t.set_shard(0, 1, 64)                                        # (one rank: the whole frame, allowed)
    still_renders("after refused shards")
    with pytest.raises(cabi.VfError, match="render_batch on a supersampled handle"):
        t.render_batch(np.stack([u, u]))
    with pytest.raises(cabi.VfError, match="render_batch on a supersampled handle"):
        t.render_batch_host(np.stack([u, u]))
    t.set_uniforms(u)
    still_renders("after refused batches")
    with pytest.raises(cabi.VfError, match="occluding overlay layers are not supported"):
        t.add_contours(np.array([0.0], F32), occlude=True)
    still_renders("after a refused occluding contour layer")
    t.close()
    # ... and through the classes
    s = scene(vf, W, H, f, h)
    assert_same(s.render_rgba(), want, "scene")
    pts = np.array([(0.0, 0.2, 0.0)], F32)
    with pytest.raises(RuntimeError, match="occluding overlay layers are not supported"):
        s.add_points(pts, occlude=True)
    with pytest.raises(RuntimeError, match="occluding overlay layers are not supported"):
        s.add_contours([0.0], occlude=True)
    assert_same(s.render_rgba(), want, "scene after refused occluding layers")         # (no layer was left behind)
    with pytest.raises(RuntimeError, match="supersampled"):
        s.render_batch([CAMERAS["default"], CAMERAS["grazing"]])
    with pytest.raises(RuntimeError, match="supersampled"):
        s.set_shard(0, 2, 64)
    s.set_camera_look_at(*CAMERAS["default"])
    assert_same(s.render_rgba(), want, "scene after refused batch and shard")
    layer = s.add_points(pts, size_px=6.0, rgba=(255, 0, 0, 255))
    with pytest.raises(RuntimeError, match="occluding overlay layers are not supported"):
        s.set_layer_occlusion(layer, True)
    s.set_layer_occlusion(layer, False)                          # (turning it off is no request for occlusion)
    s.clear_overlays()
    assert_same(s.render_rgba(), want, "scene after a refused set_layer_occlusion")
