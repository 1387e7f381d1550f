"""Anisotropic filtering of the drape's mip sampling on the GPU equals the CPU model (tests/drape_aniso_model) bit for
bit: frames for three cameras, two sizes, every anisotropy, both shade modes, both precisions, both filters, three biases, two
opacities, image sizes from one texel to the limit strips, with cast shadows and ambient occlusion, under overlays, through the
clipper, on a supersampled handle; anisotropy 1 and mipmaps off are the frames they were; the setting is the handle's, builds no
pyramid and moves nothing else."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import drape_aniso_model as dam
import occlusion_model as ocm
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from support import bits, vf, viridis  # noqa: F401
from test_gpu_drape import assert_draped, assert_frame, overlay_calls
from test_gpu_drape_mips import sized_image, sweep_case

dmm = dam.dmm
drm = dmm.drm
abm, shm = drm.abm, drm.shm
AS = (2, 4, 8, 16)


def model(u, W, H, h, mode, img, A, **kw):
    rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
    frame, again = dam.frame(rgba, vis, u, h, GRID, viridis(), img, shade_mode=1 if mode == "spec_t32" else 0, max_anisotropy=A, **kw)
    return frame, again, vis


def mip_model(u, W, H, h, mode, img, **kw):
    rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
    frame, again = dmm.frame(rgba, vis, u, h, GRID, viridis(), img, shade_mode=1 if mode == "spec_t32" else 0, **kw)
    return frame, again, vis


def aniso_scene(vf, W, H, h, cam, precision, A, bias=0.0):
    s = scene(vf, W, H, h, cam, precision)
    s.set_drape_mipmaps(True, bias=bias)
    s.set_drape_anisotropy(A)
    assert s.drape_anisotropy() == A
    return s


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, mode, A):
    W, H = 257, 131
    h = heights()
    img = dmm.case_image()
    ext = dam.CASE_EXTENT[cam]
    cases = [dict(extent=ext, opacity=opacity, filter=filt, bias=bias) for filt in ("linear", "nearest") for bias in (-1.0, 0.0, 1.5)
             for opacity in (1.0, 0.37)]
    want = {}
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        plain = s.render_rgba().copy()
        u = s.debug_uniforms_f32()
        s.set_drape_anisotropy(A)
        s.set_drape(img, extent=ext)
        for k, kw in enumerate(cases):
            kw = dict(kw)
            bias = kw.pop("bias")
            s.set_drape_mipmaps(True, bias=bias)
            s.set_drape(img, **kw)
            if k not in want:
                want[k] = model(u, W, H, h, mode, img, A, bias=bias, **kw)
                assert want[k][1].any()
            got = assert_draped(s, plain, precision, want[k], f"{precision} {cam} {mode} A = {A} case {k}")
            assert (got != plain).any() and np.array_equal(s.render_rgba(), got)
        assert s.drape_anisotropy() == A
        s.clear_drape()
        assert np.array_equal(s.render_rgba(), plain)


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_the_larger_frame(vf, cam):
    W, H = 640, 363
    h = heights()
    img = dmm.case_image()
    kw = dict(extent=dam.CASE_EXTENT[cam], opacity=0.37, filter="linear")
    s = aniso_scene(vf, W, H, h, cam, "exact", 16, bias=0.25)
    plain = s.render_rgba().copy()
    u = s.debug_uniforms_f32()
    s.set_drape(img, **kw)
    assert_draped(s, plain, "exact", model(u, W, H, h, "reference", img, 16, bias=0.25, **kw), f"{cam} {W} x {H}")


@pytest.mark.parametrize("isize", [(1, 1), (37, 53), (16384, 2), (2, 16384)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_sizes_and_extents(vf, isize):
    """the clamps of the taps (interior extent), the 64-bit texel indices and the top level (the strips)"""
    W, H = 257, 131
    h = heights()
    img = sized_image(isize)
    extents = {"full": None, "interior": dam.INTERIOR_EXTENT, "overhanging": drm.EXTENT}
    for cam in ("fill", "near"):
        s = aniso_scene(vf, W, H, h, cam, "exact", 16)
        u = s.debug_uniforms_f32()
        plain = s.render_rgba().copy()
        for name, ext in extents.items():
            for filt in ("linear", "nearest"):
                s.set_drape(img, extent=ext, filter=filt)
                want = model(u, W, H, h, "reference", img, 16, extent=ext, filter=filt, bias=0.0)
                assert want[1].any()
                assert_draped(s, plain, "exact", want, f"{isize} {cam} {name} {filt}")


@pytest.mark.parametrize("features", ["shadows", "ambient", "both"])
@pytest.mark.parametrize("cam,mode", [("default", "reference"), ("near", "reference"), ("fill", "spec_t32")])
def test_with_shadows_and_ambient_occlusion(vf, cam, mode, features):
    W, H, A = 257, 131, 8
    h = abm.scene_heights()
    shadows, ambient = features != "ambient", features != "shadows"
    strength = abm.SCENE_PARAMS["strength"]
    kw = dict(extent=dam.CASE_EXTENT[cam], opacity=0.37, filter="linear")
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
        s.set_drape_anisotropy(A)
        s.set_drape(dmm.case_image(), **kw)
        if want is None:
            lit = shm.field(u, h, GRID, **abm.SCENE_SHADOWS) if shadows else None
            sky = abm.field(u, h, GRID, abm.scene_directions(), abm.SCENE_PARAMS["reach"]) if ambient else None
            rgba, vis = support.oracle_frame(u, W, H, GRID, h, mode)
            base, _ = abm.frame(rgba, vis, u, h, GRID, viridis(), sky if ambient else np.ones((GRID, GRID), np.float32), strength, lit=lit,
                                shade_mode=1 if mode == "spec_t32" else 0)
            frame, again, smp = dam.frame(base, vis, u, h, GRID, viridis(), dmm.case_image(), lit=lit, sky=sky, strength=strength, bias=0.5,
                                          shade_mode=1 if mode == "spec_t32" else 0, max_anisotropy=A, want_sample=True, **kw)
            assert again.any() and (base != rgba).any() and (frame != base).any() and (smp[..., 7][again] > 1).any()
            want = (frame, again, vis)
        assert_draped(s, before, precision, want, f"{precision} {cam} {mode} {features}")
        s.clear_drape()
        assert np.array_equal(s.render_rgba(), before)


def test_overlays_composite_over_the_filtered_frame(vf):
    """overlay_calls holds occluding layers: they read the visibility the drape's pass reads"""
    W, H = 257, 131
    h = heights()
    for cam in ("default", "near"):
        kw = dict(extent=dam.CASE_EXTENT[cam], opacity=1.0, filter="linear")
        s = aniso_scene(vf, W, H, h, cam, "exact", 16)
        u = s.debug_uniforms_f32()
        s.set_drape(dmm.case_image(), **kw)
        calls = overlay_calls()
        assert any(c[2].get("occlude") for c in calls)
        L = apply(vf, s, calls, ocm.Layers())
        base, again, vis = model(u, W, H, h, "reference", dmm.case_image(), 16, bias=0.0, **kw)
        want = ocm.composite(base, vis, u, h, GRID, L)
        assert again.any() and (want != base).any()
        assert_frame(s.render_rgba(), want, f"overlays over the filtered drape, {cam}")


def test_the_clipped_instantiation_runs(vf):
    """the `near` camera's frame holds primitives cut by the near plane, and pixels of theirs take several taps: k_relight<true, kDrapeAniso>"""
    W, H = 257, 131
    h = heights()
    s = aniso_scene(vf, W, H, h, "near", "exact", 8, bias=0.25)
    u = s.debug_uniforms_f32()
    rgba, vis = support.oracle_frame(u, W, H, GRID, h, "reference")
    cut = dam.clipped_mask(vis, u, h, GRID)
    assert cut.any()
    for filt in ("linear", "nearest"):
        kw = dict(extent=dam.CASE_EXTENT["near"], filter=filt)
        s.set_drape(dmm.case_image(), **kw)
        frame, again, smp = dam.frame(rgba, vis, u, h, GRID, viridis(), dmm.case_image(), bias=0.25, max_anisotropy=8, want_sample=True, **kw)
        assert (smp[..., 7][cut & again] > 1).any()
        assert_draped(s, rgba, "exact", (frame, again, vis), f"near {filt}")


def test_anisotropy_1_and_mipmaps_off_are_the_frames_they_were(vf):
    W, H = 257, 131
    h = heights()
    img = dmm.case_image()
    for cam in ("default", "fill"):
        kw = dict(extent=dam.CASE_EXTENT[cam], opacity=0.37, filter="linear")
        s = scene(vf, W, H, h, cam, "exact")
        u = s.debug_uniforms_f32()
        assert s.drape_anisotropy() == 1
        s.set_drape(img, **kw)
        flat = s.render_rgba().copy()
        s.set_drape_anisotropy(16)                             # mipmaps off: kept, and no effect
        assert s.drape_anisotropy() == 16 and s.drape_mip_info() is None and np.array_equal(s.render_rgba(), flat)
        s.set_drape_anisotropy(1)
        s.set_drape_mipmaps(True, bias=0.5)
        mipped = s.render_rgba().copy()
        assert (mipped != flat).any()
        assert_frame(mipped, mip_model(u, W, H, h, "reference", img, bias=0.5, **kw)[0], f"mipped {cam}")
        builds = s.drape_mip_info()["builds"]
        assert builds == 1
        s.set_drape_anisotropy()                               # the default is 1
        assert s.drape_anisotropy() == 1 and np.array_equal(s.render_rgba(), mipped)
        frames = {}
        for A in AS:                                          # up ...
            s.set_drape_anisotropy(A)
            frames[A] = s.render_rgba().copy()
            assert (frames[A] != mipped).any(), A
            assert_frame(frames[A], model(u, W, H, h, "reference", img, A, bias=0.5, **kw)[0], f"{cam} A = {A}")
        assert all((frames[a] != frames[b]).any() for a in AS for b in AS if a < b)
        for A in (8, 1, 16, 2, 1, 4):                         # ... and back and forth: the same frames, and no pyramid is built
            s.set_drape_anisotropy(A)
            assert s.drape_anisotropy() == A and np.array_equal(s.render_rgba(), mipped if A == 1 else frames[A]), A
        assert s.drape_mip_info()["builds"] == builds
        # the setting survives mipmaps off / on, set_drape and clear_drape
        s.set_drape_anisotropy(8)
        s.set_drape_mipmaps(False)
        assert s.drape_anisotropy() == 8 and np.array_equal(s.render_rgba(), flat)
        s.set_drape_mipmaps(True, bias=0.5)
        assert s.drape_anisotropy() == 8 and np.array_equal(s.render_rgba(), frames[8])
        s.set_drape(img, **kw)
        assert s.drape_anisotropy() == 8 and np.array_equal(s.render_rgba(), frames[8])
        s.clear_drape()
        assert s.drape_anisotropy() == 8
        s.set_drape(img, **kw)
        assert s.drape_anisotropy() == 8 and np.array_equal(s.render_rgba(), frames[8])
        assert s.drape_mip_info()["builds"] == builds + 3      # (one per image set or enabling, none for the setting)


def test_nothing_else_moves(vf):
    W, H = 257, 131
    h = heights(5)
    never = scene(vf, W, H, h, "near")
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    vis = never.debug_visibility().copy()
    s = scene(vf, W, H, h, "near")
    s.set_drape_mipmaps(True, bias=1.0)
    s.set_drape_anisotropy(16)
    assert np.array_equal(s.render_rgba(), want)               # the setting without a drape: the plain frame
    s.set_drape(dmm.case_image(), extent=dam.CASE_EXTENT["near"])
    draped = s.render_rgba().copy()
    assert (draped != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.debug_visibility(), vis)
    assert np.array_equal(s.render_rgba(), draped)
    assert s.drape_mip_info()["bias"] == 1.0 and s.drape_anisotropy() == 16
    s.clear_drape()
    assert np.array_equal(s.render_rgba(), want)


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    W, H = 128, 128
    h = heights(2, (32, 32))
    img = dmm.case_image()
    u = support.uniforms(W, H)
    t = cabi.Terrain(W, H, 32, viridis())
    t.set_height(h)
    t.set_uniforms(u)
    t.set_drape_mipmaps(True, bias=0.5)
    t.set_drape_anisotropy(4)
    t.set_drape(img, extent=drm.EXTENT)
    t.render()
    draped = t.read_rgba().copy()
    info = t.drape_mip_info()
    for bad in (0, 3, 5, 12, 17, 32, 2 ** 32 - 1):
        assert t.lib.vf_terrain_set_drape_anisotropy(t.t, bad) == cabi.VF_ERR_INVALID, bad
        assert "1, 2, 4, 8 or 16" in t.lib.vf_last_error().decode()
        assert t.drape_anisotropy() == 4 and t.drape_mip_info() == info
    assert t.lib.vf_terrain_drape_anisotropy(t.t, None) == cabi.VF_ERR_INVALID
    for bad, err in ((3, ValueError), (True, TypeError), (4.0, TypeError), ("4", TypeError)):
        with pytest.raises(err, match="max_anisotropy"):
            t.set_drape_anisotropy(bad)
    assert t.lib.vf_terrain_set_shard(t.t, 0, 2, 64) == cabi.VF_ERR_INVALID and "draped image" in t.lib.vf_last_error().decode()
    with pytest.raises(RuntimeError, match="render_batch on a handle that holds a draped image"):
        t.render_batch(np.stack([u, u]))
    t.render()
    assert np.array_equal(t.read_rgba(), draped) and t.drape_anisotropy() == 4
    assert t.drape_stage(2) > 0 and t.drape_mip_info() == info      # (the diagnostic times the pass the handle runs)
    t.render()
    assert np.array_equal(t.read_rgba(), draped)
    t.close()
    s = scene(vf, W, H, h)
    s.set_drape_anisotropy(2)
    for bad, err in ((3, ValueError), (0, ValueError), (True, TypeError), (2.0, TypeError), ("2", TypeError), (None, TypeError)):
        with pytest.raises(err, match="max_anisotropy"):
            s.set_drape_anisotropy(bad)
    assert s.drape_anisotropy() == 2


def test_through_the_c_abi_and_the_spike(vf):
    from vulkan_forge_amd import cabi
    import oracle
    W, H, grid = 129, 97, 48
    rng = np.random.default_rng(3)
    tex = (rng.random((23, 31), dtype=np.float32) * 0.5 - 0.25).astype(np.float32)
    img = dmm.case_image()
    kw = dict(extent=(-2.0, -9.0, 2.2, 9.5), opacity=0.8, filter="linear")
    u = support.uniforms(W, H)
    rgba, vis = oracle.render_terrain(u, W, H, grid, tex, viridis(), want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    rgba = rgba.reshape(H, W, 4)
    t = cabi.Terrain(W, H, grid, viridis())
    t.set_height(tex)
    t.set_shade_precision(0)
    t.set_uniforms(u)
    assert t.drape_anisotropy() == 1
    t.set_drape_mipmaps(True, bias=0.0)
    t.set_drape(img, **kw)
    for A in (16, 1, 4):
        t.set_drape_anisotropy(A)
        assert t.drape_anisotropy() == A
        t.render()
        want, again, smp = dam.frame(rgba, vis, u, tex, grid, viridis(), img, bias=0.0, max_anisotropy=A, want_sample=True, **kw)
        assert again.any() and (A == 1 or (smp[..., 7][again] > 1).any())
        assert_frame(t.read_rgba().copy(), want, f"cabi.Terrain A = {A}")
        assert np.array_equal(t.read_visibility(), vis)
    assert t.drape_mip_info()["builds"] == 1
    t.close()
    Ws, Hs, G = 160, 120, 48
    sp = vf.TerrainSpike(Ws, Hs, grid=G)
    sp.set_shade_precision("exact")
    assert sp.drape_anisotropy() == 1
    plain = sp.render_rgba().copy()
    us = sp.debug_uniforms_f32()
    srgba, svis = oracle.render_terrain(us, Ws, Hs, G, oracle.SPIKE_DUMMY_HEIGHT, viridis(), want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    srgba = srgba.reshape(Hs, Ws, 4)
    assert_frame(plain, srgba, "the spike's plain frame")
    sp.set_drape_mipmaps(True)
    sp.set_drape_anisotropy(8)
    skw = dict(extent=(-1.5, -6.0, 1.5, 6.0))
    sp.set_drape(img, **skw)
    want, again, smp = dam.frame(srgba, svis, us, oracle.SPIKE_DUMMY_HEIGHT, G, viridis(), img, max_anisotropy=8, want_sample=True, **skw)
    assert again.any() and (smp[..., 7][again] > 1).any()
    assert sp.drape_anisotropy() == 8
    assert_frame(sp.render_rgba().copy(), want, "TerrainSpike A = 8")
    sp.clear_drape()
    assert np.array_equal(sp.render_rgba(), plain) and sp.drape_anisotropy() == 8


def test_a_supersampled_handle_filters_its_samples(vf):
    import oracle
    W, H, f = 129, 97, 2
    h = heights()
    img = dmm.case_image()
    kw = dict(extent=dam.CASE_EXTENT["default"], opacity=0.37, filter="linear")
    s = vf.Scene(W, H, grid=GRID, supersample=f)
    s.set_height_from_r32f(h)
    s.set_shade_precision("exact")
    s.set_camera_look_at(*CAMERAS["default"])
    u = s.debug_uniforms_f32()
    s.set_drape_mipmaps(True, bias=0.0)
    s.set_drape_anisotropy(16)
    s.set_drape(img, **kw)
    s.render_rgba()
    samples = s.render_samples()
    assert samples.shape == (f * H, f * W, 4)
    rgba, vis = oracle.render_terrain(u, f * W, f * H, GRID, h, viridis(), want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    want, again, smp = dam.frame(rgba.reshape(f * H, f * W, 4), vis, u, h, GRID, viridis(), img, bias=0.0, max_anisotropy=16, want_sample=True, **kw)
    assert again.any() and (smp[..., 7][again] > 1).any()
    assert_frame(samples, want, "samples of a supersampled handle")
    mipped, _ = dmm.frame(rgba.reshape(f * H, f * W, 4), vis, u, h, GRID, viridis(), img, bias=0.0, **kw)
    assert (want != mipped).any()


@pytest.mark.parametrize("k", range(24))
def test_a_seeded_sweep(k):
    """the mip sweep's cases (image sizes 1 ... 300, extents, biases, filters, cameras, spacings, one NaN texel) with a random anisotropy
    and an extent stretched along one axis"""
    import oracle
    from vulkan_forge_amd import cabi
    W, H, grid, tex, u, img, kw = sweep_case(k)
    rng = np.random.default_rng(5000 + k)
    A = int(rng.choice(AS))
    x0, z0, x1, z1 = kw["extent"]
    stretch = float(rng.choice([1.0, 3.0, 9.0]))
    kw["extent"] = (x0, z0, x0 + (x1 - x0) * stretch, z1) if rng.random() < 0.5 else (x0, z0, x1, z0 + (z1 - z0) * stretch)
    rgba, vis = oracle.render_terrain(u, W, H, grid, tex, viridis(), want_vis=True, nthreads=8, shade_mode=oracle.SHADE_REFERENCE)
    rgba = rgba.reshape(H, W, 4)
    want, again, smp = dam.frame(rgba, vis, u, tex, grid, viridis(), img, max_anisotropy=A, want_sample=True, **kw)
    n = smp[..., 7][again]
    print(f"case {k}: A = {A}, image {img.shape[1]} x {img.shape[0]}, grid {grid}, {kw}, {int(again.sum())} of {int((vis != 0).sum())} covered pixels "
          f"rewritten, mean N {n.mean():.2f}, {int(smp[..., 9][again].sum())} with a clamped tap")
    assert again.any() and (n > 1).any()
    t = cabi.Terrain(W, H, grid, viridis())
    t.set_height(tex)
    t.set_shade_precision(0)
    t.set_uniforms(u)
    bias = kw.pop("bias")
    t.set_drape_mipmaps(True, bias=bias)
    t.set_drape_anisotropy(A)
    t.set_drape(img, **kw)
    t.render()
    got = t.read_rgba().copy()
    assert np.array_equal(t.read_visibility(), vis)
    assert_frame(got, want, f"sweep case {k}")
    t.close()
