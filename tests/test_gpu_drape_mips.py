"""The drape's mip pyramid and trilinear filtering on the GPU equal the CPU model (tests/drape_mip_model) bit for bit:
the pyramid at every level, frames for three cameras, two sizes, both shade modes, both precisions, both filters, three biases,
two opacities, image sizes from one texel to the limit strips, with cast shadows and ambient occlusion, under overlays, through the
clipper; mipmaps at bias -16 and mipmaps off are the unmipped drape; the pyramid is built once per image; nothing else moves."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import drape_mip_model as dmm
import occlusion_model as ocm
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from support import bits, vf, viridis  # noqa: F401
from test_gpu_drape import assert_draped, assert_frame, overlay_calls

drm = dmm.drm
abm, shm = drm.abm, drm.shm
SIZES = [(257, 131), (640, 363)]
PYRAMID_SIZES = [(37, 53), (1, 1), (2, 3), (5, 1), (211, 157), (16384, 2), (2, 16384), dmm.CASE_SIZE]


def model(u, W, H, h, mode, img, **kw):
    rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
    frame, again = dmm.frame(rgba, vis, u, h, GRID, viridis(), img, shade_mode=1 if mode == "spec_t32" else 0, **kw)
    return frame, again, vis


def flat_model(u, W, H, h, mode, img, **kw):
    rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
    frame, again = drm.frame(rgba, vis, u, h, GRID, viridis(), img, shade_mode=1 if mode == "spec_t32" else 0, **kw)
    return frame, again, vis


def sized_image(isize):
    if isize == dmm.CASE_SIZE:
        return dmm.case_image()
    img = drm.image(seed=isize[0] * 7 + isize[1], size=isize)
    if not img[..., 3].any():
        img[..., 3] = np.random.default_rng(2).integers(1, 256, img.shape[:2], dtype=np.uint8)
    return img


@pytest.mark.parametrize("channels", [4, 3])
@pytest.mark.parametrize("isize", PYRAMID_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_pyramid_equals_the_model_at_every_level(vf, isize, channels):
    s = vf.Scene(64, 48, grid=32)
    s.set_drape_mipmaps(True)
    info = s.drape_mip_info()
    assert info == {"levels": 0, "sizes": [], "bias": 0.0, "bytes": 0, "builds": 0}
    img = sized_image(isize)[..., :channels].copy()
    s.set_drape(img)
    want = dmm.pyramid(img)
    info = s.drape_mip_info()
    assert info["levels"] == len(want) and info["sizes"] == dmm.sizes(*isize) and info["builds"] == 0
    assert info["bytes"] >= 8 * sum(w * h for w, h in info["sizes"][1:]) and info["bytes"] <= 8 * sum(w * h + 1 for w, h in info["sizes"][1:])
    for k in range(1, len(want)):
        got = s.read_drape_level(k)
        assert got.dtype == np.float16 and got.shape == want[k].shape, k
        d = got.view(np.uint16) != want[k].view(np.uint16)
        assert not d.any(), f"level {k}: {int(d.sum())} values differ, first at {np.argwhere(d)[:4].tolist()}"
    assert s.drape_mip_info()["builds"] == (1 if len(want) > 1 else 0)
    for bad in (0, len(want), -1):
        with pytest.raises(ValueError, match="level"):
            s.read_drape_level(bad)


@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, size, mode):
    W, H = size
    h = heights()
    img = dmm.case_image()
    ext = dmm.CASE_EXTENT[cam]
    cases = [dict(extent=ext, opacity=1.0, filter="linear", bias=0.0), dict(extent=ext, opacity=0.37, filter="nearest", bias=0.0),
             dict(extent=ext, opacity=0.37, filter="linear", bias=1.5), dict(extent=ext, opacity=1.0, filter="nearest", bias=-1.0),
             dict(extent=ext, opacity=1.0, filter="linear", bias=-1.0), dict(extent=ext, opacity=0.37, filter="nearest", bias=1.5)]
    want = {}
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        plain = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
        s.set_drape(img, extent=ext)
        for k, kw in enumerate(cases):
            kw = dict(kw)
            bias = kw.pop("bias")
            s.set_drape_mipmaps(True, bias=bias)
            s.set_drape(img, **kw)
            if k not in want:
                want[k] = model(u, W, H, h, mode, img, bias=bias, **kw)
                assert want[k][1].any()
            got = assert_draped(s, plain, precision, want[k], f"{precision} {cam} {size} {mode} case {k}")
            assert (got != plain).any() and np.array_equal(s.render_rgba(), got)
        assert s.drape_mip_info()["builds"] == len(cases)     # one per image set, none per frame or per bias
        s.clear_drape()
        assert np.array_equal(s.render_rgba(), plain) and s.drape_mip_info()["levels"] == 0


@pytest.mark.parametrize("isize", [(1, 1), (37, 53), (16384, 2), (2, 16384)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_sizes_and_extents(vf, isize):
    W, H = 257, 131
    h = heights()
    img = sized_image(isize)
    extents = {"full": None, "interior": (-0.7, -0.5, 0.9, 0.8), "overhanging": drm.EXTENT}
    for cam in ("fill", "near"):
        s = scene(vf, W, H, h, cam, "exact")
        s.set_drape_mipmaps(True, bias=0.0)
        u = s.debug_uniforms_f32()
        plain = s.render_rgba().copy()
        for name, ext in extents.items():
            for filt in ("linear", "nearest"):
                s.set_drape(img, extent=ext, filter=filt)
                want = model(u, W, H, h, "reference", img, extent=ext, filter=filt, bias=0.0)
                assert want[1].any()
                assert_draped(s, plain, "exact", want, f"{isize} {cam} {name} {filt}")


@pytest.mark.parametrize("features", ["shadows", "ambient", "both"])
@pytest.mark.parametrize("cam,mode", [("default", "reference"), ("near", "reference"), ("fill", "spec_t32")])
def test_with_shadows_and_ambient_occlusion(vf, cam, mode, features):
    W, H = 257, 131
    h = abm.scene_heights()
    shadows, ambient = features != "ambient", features != "shadows"
    strength = abm.SCENE_PARAMS["strength"]
    kw = dict(extent=dmm.CASE_EXTENT[cam], opacity=0.37, filter="linear")
    want = None
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        s.set_sun(*abm.SCENE_SUN_DEG)
        s.set_shadows(shadows, **abm.SCENE_SHADOWS)
        s.set_ambient_occlusion(ambient, strength=strength, reach=abm.SCENE_PARAMS["reach"], directions=abm.scene_directions())
        before = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
        s.set_drape_mipmaps(True, bias=0.5)
        s.set_drape(dmm.case_image(), **kw)
        if want is None:
            lit = shm.field(u, h, GRID, **abm.SCENE_SHADOWS) if shadows else None
            sky = abm.field(u, h, GRID, abm.scene_directions(), abm.SCENE_PARAMS["reach"]) if ambient else None
            rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
            base, _ = abm.frame(rgba, vis, u, h, GRID, viridis(), sky if ambient else np.ones((GRID, GRID), np.float32), strength, lit=lit,
                                shade_mode=1 if mode == "spec_t32" else 0)
            frame, again = dmm.frame(base, vis, u, h, GRID, viridis(), dmm.case_image(), lit=lit, sky=sky, strength=strength, bias=0.5,
                                     shade_mode=1 if mode == "spec_t32" else 0, **kw)
            assert again.any() and (base != rgba).any() and (frame != base).any()
            want = (frame, again, vis)
        assert_draped(s, before, precision, want, f"{precision} {cam} {mode} {features}")
        s.clear_drape()
        assert np.array_equal(s.render_rgba(), before)


def test_overlays_composite_over_the_mipped_frame(vf):
    W, H = 257, 131
    h = heights()
    for cam in ("default", "near"):
        kw = dict(extent=dmm.CASE_EXTENT[cam], opacity=1.0, filter="linear")
        s = scene(vf, W, H, h, cam, "exact")
        u = s.debug_uniforms_f32()
        s.set_drape_mipmaps(True)
        s.set_drape(dmm.case_image(), **kw)
        L = apply(vf, s, overlay_calls(), ocm.Layers())
        base, again, vis = model(u, W, H, h, "reference", dmm.case_image(), bias=0.0, **kw)
        want = ocm.composite(base, vis, u, h, GRID, L)
        assert again.any() and (want != base).any()
        assert_frame(s.render_rgba(), want, f"overlays over the mipped drape, {cam}")


def test_the_clipped_instantiation_runs(vf):
    """the `near` camera's frame holds primitives cut by the near plane (their ids are in the visibility): k_relight<true, kDrapeMip>"""
    W, H = 257, 131
    h = heights()
    s = scene(vf, W, H, h, "near", "exact")
    u = s.debug_uniforms_f32()
    rgba, vis = support.oracle_frame(u, W, H, GRID, h, "reference")
    assert dmm.clipped_pixels(vis, u, h, GRID) > 0
    s.set_drape_mipmaps(True, bias=0.25)
    for filt in ("linear", "nearest"):
        s.set_drape(dmm.case_image(), extent=dmm.CASE_EXTENT["near"], filter=filt)
        want = model(u, W, H, h, "reference", dmm.case_image(), extent=dmm.CASE_EXTENT["near"], filter=filt, bias=0.25)
        assert_draped(s, rgba, "exact", want, f"near {filt}")


def test_bias_minus_16_and_mipmaps_off_are_the_unmipped_drape(vf):
    W, H = 257, 131
    h = heights()
    img = dmm.case_image()
    for cam in ("default", "near"):
        kw = dict(extent=dmm.CASE_EXTENT[cam], opacity=0.37, filter="linear")
        s = scene(vf, W, H, h, cam, "exact")
        u = s.debug_uniforms_f32()
        plain = s.render_rgba().copy()
        s.set_drape(img, **kw)
        assert s.drape_mip_info() is None
        flat = s.render_rgba().copy()
        assert_frame(flat, flat_model(u, W, H, h, "reference", img, **kw)[0], f"unmipped {cam}")
        s.set_drape_mipmaps(True, bias=-16.0)
        assert np.array_equal(s.render_rgba(), flat)
        s.set_drape_mipmaps(True, bias=0.0)
        mipped = s.render_rgba().copy()
        assert (mipped != flat).any()
        assert_frame(mipped, model(u, W, H, h, "reference", img, bias=0.0, **kw)[0], f"mipped {cam}")
        builds = s.drape_mip_info()["builds"]
        assert builds == 1
        # on -> off -> on, clear -> set: the same frames again
        s.set_drape_mipmaps(False)
        assert s.drape_mip_info() is None and np.array_equal(s.render_rgba(), flat)
        with pytest.raises(ValueError, match="level"):
            s.read_drape_level(1)
        s.set_drape_mipmaps(True)
        assert np.array_equal(s.render_rgba(), mipped) and s.drape_mip_info()["builds"] == builds + 1
        s.clear_drape()
        info = s.drape_mip_info()
        assert info["levels"] == 0 and info["sizes"] == [] and np.array_equal(s.render_rgba(), plain)
        s.set_drape(img, **kw)
        assert np.array_equal(s.render_rgba(), mipped) and s.drape_mip_info()["builds"] == builds + 2
        for _ in range(3):
            assert np.array_equal(s.render_rgba(), mipped)
        s.set_camera_look_at(*CAMERAS["fill"])
        s.render_rgba()
        assert s.drape_mip_info()["builds"] == builds + 2      # a resting image is not reduced again


def test_nothing_else_moves(vf):
    W, H = 257, 131
    h = heights(5)
    never = scene(vf, W, H, h, "near")
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    vis = never.debug_visibility().copy()
    s = scene(vf, W, H, h, "near")
    s.set_drape_mipmaps(True, bias=1.0)
    assert np.array_equal(s.render_rgba(), want)               # mipmaps on without a drape: the plain frame
    s.set_drape(dmm.case_image(), extent=dmm.CASE_EXTENT["near"])
    draped = s.render_rgba().copy()
    assert (draped != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), vis)
    assert np.array_equal(s.render_rgba(), draped)
    assert s.drape_mip_info()["bias"] == 1.0
    s.clear_drape()
    assert np.array_equal(s.render_rgba(), want)
    sp = vf.TerrainSpike(160, 120, grid=48)
    spike = sp.render_rgba().copy()
    sp.set_drape_mipmaps(True)
    sp.set_drape(drm.opaque_image((64, 64)))
    assert sp.drape_mip_info()["levels"] == 7 and (sp.render_rgba() != spike).any()
    sp.clear_drape()
    assert np.array_equal(sp.render_rgba(), spike)


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    W, H = 128, 128
    h = heights(2, (32, 32))
    img = drm.image()
    u = support.uniforms(W, H)
    t = cabi.Terrain(W, H, 32, viridis())
    t.set_height(h)
    t.set_uniforms(u)
    t.set_drape_mipmaps(True, bias=0.5)
    t.set_drape(img, extent=drm.EXTENT)
    t.render()
    draped = t.read_rgba().copy()
    info = t.drape_mip_info()
    assert info["levels"] == 7 and info["bias"] == 0.5 and info["builds"] == 1
    nan, inf = float("nan"), float("inf")
    for bad in (nan, inf, -inf, 16.5, -16.001):
        assert t.lib.vf_terrain_set_drape_mips(t.t, 1, bad) == cabi.VF_ERR_INVALID, bad
        assert t.lib.vf_terrain_set_drape_mips(t.t, 0, bad) == cabi.VF_ERR_INVALID, bad
        assert t.drape_mip_info() == info
    w, hh = cabi.C.c_uint32(), cabi.C.c_uint32()
    for bad in (0, 7, 100):
        assert t.lib.vf_terrain_read_drape_level(t.t, bad, None, cabi.C.byref(w), cabi.C.byref(hh)) == cabi.VF_ERR_INVALID
    assert t.lib.vf_terrain_set_shard(t.t, 0, 2, 64) == cabi.VF_ERR_INVALID and "draped image" in t.lib.vf_last_error().decode()
    with pytest.raises(RuntimeError, match="render_batch on a handle that holds a draped image"):
        t.render_batch(np.stack([u, u]))
    t.render()
    assert np.array_equal(t.read_rgba(), draped) and t.drape_mip_info() == info
    assert t.drape_stage(2) > 0 and t.drape_mip_info() == info
    assert t.drape_mip_build_stage(2) > 0 and t.drape_mip_info() == info      # (diagnostic builds are not the handle's)
    t.render()
    assert np.array_equal(t.read_rgba(), draped)
    t.close()
    s = scene(vf, W, H, h)
    for bad, err in ((17.0, ValueError), (nan, ValueError), ("soft", TypeError)):
        with pytest.raises(err, match="bias"):
            s.set_drape_mipmaps(True, bias=bad)
    assert s.drape_mip_info() is None
    s.set_drape_mipmaps(True)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_drape(img)
    s.set_shard(0, 1, 64)
    s.set_drape(img)
    with pytest.raises(RuntimeError, match="render_batch on a handle that holds a draped image"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])


def test_the_image_from_device_memory_on_a_stream_of_the_callers():
    support.run_check("drape_mip_torch_check.py", "DRAPE MIP TORCH OK")


def sweep_case(k):
    """case k of the seeded sweep: image sizes 1 ... 300 (odd edges at every level), extents, biases, filters, cameras, spacings, a
    NaN texel in the height texture"""
    import oracle
    rng = np.random.default_rng(1000 + k)
    W, H, grid = 129, 97, int(rng.choice([24, 33, 48]))
    spacing = float(rng.choice([0.25, 1.0, 2.0]))
    tex = (rng.random((int(rng.integers(9, 40)), int(rng.integers(9, 40))), dtype=np.float32) * 0.5 - 0.25).astype(np.float32)
    tex[int(rng.integers(0, tex.shape[0])), int(rng.integers(0, tex.shape[1]))] = np.nan
    eye, at, up, fov, near, far = CAMERAS[("default", "fill", "near")[k % 3]]
    if k % 3 != 2:                                            # further out with the terrain's width
        cam = (tuple(v * spacing for v in eye), at, up, fov, near * min(1.0, spacing), far)
    else:                                                     # the whole view scaled: the terrain still passes through the near plane
        cam = (tuple(v * spacing for v in eye), tuple(v * spacing for v in at), up, fov, near * spacing, far)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *cam), np.float32).reshape(44)
    u[36] = spacing
    iw, ih = int(rng.integers(1, 301)), int(rng.integers(1, 301))
    img = rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)
    img[rng.random((ih, iw)) < 0.2, 3] = 0
    img[rng.random((ih, iw)) < 0.3, 3] = 255
    x0, z0 = rng.uniform(-2.0, 0.2, 2)                        # (every camera sees a part of the extent: it reaches past 0.6)
    size = rng.uniform(2.6, 3.6, 2) * float(rng.choice([1.0, 4.0, 12.0]))
    ext = (float(x0), float(z0), float(x0 + size[0]), float(z0 + size[1]))
    kw = dict(extent=ext, opacity=float(rng.choice([1.0, 0.37])), filter=str(rng.choice(["linear", "nearest"])),
              bias=float(rng.choice([0.0, -1.0, 1.5, 3.0, 5.0, float(np.float32(rng.uniform(-2, 6)))])))
    return W, H, grid, tex, u, img, kw


@pytest.mark.parametrize("k", range(24))
def test_a_seeded_sweep(k):
    import oracle
    from vulkan_forge_amd import cabi
    W, H, grid, tex, u, img, kw = sweep_case(k)
    rgba, vis = oracle.render_terrain(u, W, H, grid, tex, viridis(), want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    rgba = rgba.reshape(H, W, 4)
    want, again = dmm.frame(rgba, vis, u, tex, grid, viridis(), img, **kw)
    print(f"case {k}: image {img.shape[1]} x {img.shape[0]}, grid {grid}, {kw}, {int(again.sum())} of {int((vis != 0).sum())} covered pixels rewritten")
    assert again.any()                                        # (every case's extent meets its view)
    if k % 3 == 2:                                            # the `near` cameras: primitives cut by the near plane are on screen
        assert dmm.clipped_pixels(vis, u, tex, grid) > 0
    t = cabi.Terrain(W, H, grid, viridis())
    t.set_height(tex)
    t.set_shade_precision(0)
    t.set_uniforms(u)
    bias = kw.pop("bias")
    t.set_drape_mipmaps(True, bias=bias)
    t.set_drape(img, **kw)
    t.render()
    got = t.read_rgba().copy()
    assert np.array_equal(t.read_visibility(), vis)
    assert_frame(got, want, f"sweep case {k}")
    levels = dmm.pyramid(img)
    for lv in range(1, len(levels)):
        assert np.array_equal(t.read_drape_level(lv).view(np.uint16), levels[lv].view(np.uint16)), lv
    t.close()
