"""Cast sun shadows on the GPU equal the CPU model (tests/shadow_model) bit for bit: the shadow field for suns in every
octant and on every special direction, on grids that are and are not a multiple of 8 and long enough for many chunks, through both
entry points; the shadowed frame over three cameras, two sizes, both shade modes and both precisions; with overlays on top; and
nothing else moves -- geometry buffers, the frame with shadows off, the refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import overlay_model as om
import shadow_model as shm
from overlay_scenes import CAMERAS, GRID, apply, heights, scene
from shadow_model import SCENE_PARAMS, SCENE_SUN_DEG
from support import assert_field, bits, terrain, uniforms, vf, viridis  # noqa: F401

# (x, y, z): the eight octants of the horizontal plane at general azimuths, the four axes, the exact diagonals, straight up,
# on the horizon and below it
SUNS = [(0.9, 0.5, 0.31), (0.31, 0.5, 0.9), (-0.31, 0.4, 0.9), (-0.9, 0.7, 0.31), (-0.9, 0.3, -0.31), (-0.31, 0.6, -0.9), (0.31, 0.45, -0.9), (0.9, 0.55, -0.31),
        (1.0, 0.6, 0.0), (-1.0, 0.6, 0.0), (0.0, 0.6, 1.0), (0.0, 0.6, -1.0),
        (0.5, 0.4, 0.5), (-0.5, 0.4, 0.5), (0.5, 0.4, -0.5), (-0.5, 0.4, -0.5),
        (0.0, 1.0, 0.0), (0.7, 0.0, 0.2), (0.2, -0.3, 0.7)]
PARAMS = dict(strength=0.8, softness=0.05, bias=0.01)


@pytest.mark.parametrize("grid", [1024, 1025, 203, 1500])
def test_field_equals_the_model(grid):
    h = heights(4, (97, 131))
    t = terrain(64, 64, grid, h)
    t.set_shadows(False, **PARAMS)                            # the field does not need shadows enabled for drawing
    shadowed = 0
    for sun in SUNS:
        u = uniforms(64, 64, sun=sun, exag=0.6)
        t.set_uniforms(u)
        got = t.shadow_field()
        want = shm.field(u, h, grid, **PARAMS)
        assert got.shape == (grid, grid) and got.dtype == np.float32
        assert_field(got, want, f"grid {grid} sun {sun}")
        shadowed += int((want < 1).sum())
        if sun[0] == 0.0 and sun[2] == 0.0:
            assert (got == 1).all()
    assert shadowed > grid * grid                             # (the comparison is not one of empty shadows)
    t.close()


def test_field_into_device_memory_on_a_stream_of_the_callers():
    support.run_check("shadow_torch_check.py", "SHADOW TORCH OK")


def oracle_frame(vf, u, W, H, h, mode):
    # (not support.oracle_frame: these frames go up to 1920 x 1080, and a process-wide cache should not keep twelve of them)
    import oracle
    return oracle.render_terrain(u, W, H, GRID, h, viridis(), want_vis=True, nthreads=8,
                                 shade_mode=oracle.SHADE_SPEC_T32 if mode == "spec_t32" else oracle.SHADE_REFERENCE)


def model_frame(vf, u, W, H, h, mode):
    rgba, vis = oracle_frame(vf, u, W, H, h, mode)
    lit = shm.field(u, h, GRID, **SCENE_PARAMS)
    frame, mask = shm.frame(rgba, vis, u, h, GRID, viridis(), lit, shade_mode=1 if mode == "spec_t32" else 0)
    return frame, mask, vis


def assert_frame(got, want, what, where=None):
    # byte for byte, at the pixels of the mask `where` if one is given
    support.assert_frame(got if where is None else np.where(where[..., None], got, want), want, what)


@pytest.mark.parametrize("mode", ["reference", "spec_t32"])
@pytest.mark.parametrize("size", [(1920, 1080), (257, 131)])
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model_in_both_precisions(vf, cam, size, mode):
    W, H = size
    h = heights()
    want = None
    for precision in ("exact", "fast"):
        s = scene(vf, W, H, h, cam, precision)
        s.set_shade_mode(mode)
        s.set_sun(*SCENE_SUN_DEG)
        plain = s.render_rgba().copy()
        s.set_shadows(True, **SCENE_PARAMS)
        got = s.render_rgba()
        if want is None:
            want, mask, vis = model_frame(vf, s.debug_uniforms_f32(), W, H, h, mode)
            frac = mask.sum() / max(int((vis != 0).sum()), 1)
            print(f"{cam} {W}x{H} {mode}: {frac:.3f} of the covered pixels are shadowed")
            assert 0.1 < frac < 0.9
        if precision == "exact":
            assert_frame(got, want, f"exact {cam} {size} {mode}")
        else:                                                 # shadowed pixels take the exact arithmetic, the others keep the fast frame's bytes
            assert_frame(got, want, f"fast {cam} {size} {mode}, shadowed pixels", mask)
            assert_frame(got, plain, f"fast {cam} {size} {mode}, other pixels", ~mask)
        assert (got != plain).any()
        assert np.array_equal(s.render_rgba(), got)


def test_overlays_composite_over_the_shadowed_frame(vf):
    W, H = 640, 400
    h = heights()
    s = scene(vf, W, H, h, "default", "exact")
    s.set_sun(*SCENE_SUN_DEG)
    s.set_shadows(True, **SCENE_PARAMS)
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(5)
    n = 2000
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.08, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(100)]
    poly = [np.array([[-0.6, 0.05, -0.6], [0.7, 0.05, -0.5], [0.1, 0.05, 0.8]], np.float32)]
    calls = [("add_points", (pts,), dict(size_px=5.0, rgba=(255, 0, 0, 200), drape=True)),
             ("add_lines", (paths,), dict(width_px=3.0, rgba=(0, 255, 0, 200), drape=True)),
             ("add_polygons", (poly,), dict(fill_rgba=(0, 90, 255, 160)))]
    import polygon_model as pm
    L = apply(vf, s, calls, pm.Layers())
    base, mask, _ = model_frame(vf, u, W, H, h, "reference")
    want = pm.composite(base, u, h, GRID, L)
    got = s.render_rgba()
    assert mask.any() and (want != base).any()
    assert_frame(got, want, "overlays over shadows")


def test_gbuffers_and_the_frame_with_shadows_off_are_unchanged(vf):
    W, H = 640, 400
    h = heights(5)
    never = scene(vf, W, H, h)
    never.set_sun(*SCENE_SUN_DEG)
    want = never.render_rgba().copy()
    planes = never.render_gbuffer()
    s = scene(vf, W, H, h)
    s.set_sun(*SCENE_SUN_DEG)
    assert np.array_equal(s.render_rgba(), want)              # before enabling
    s.set_shadows(True, **SCENE_PARAMS)
    shadowed = s.render_rgba().copy()
    assert (shadowed != want).any()
    g = s.render_gbuffer()
    for k in planes:
        assert np.array_equal(bits(g[k]), bits(planes[k])), k
    assert np.array_equal(s.render_rgba(), shadowed)
    s.set_shadows(False)
    assert np.array_equal(s.render_rgba(), want)              # after enable followed by disable
    # the new setters change no default: a scene that calls them with the defaults' values draws the same bytes
    a, b = scene(vf, W, H, h), scene(vf, W, H, h)
    base = a.render_rgba().copy()
    b.set_exposure(1.0)
    assert np.array_equal(b.render_rgba(), base)
    b.set_exposure(1.7)
    assert (b.render_rgba() != base).any()
    with pytest.raises(ValueError, match="exposure must be > 0"):
        b.set_exposure(0.0)
    with pytest.raises(ValueError, match="angles must be finite"):
        b.set_sun(float("nan"), 0.0)
    sp = vf.TerrainSpike(160, 120, grid=48)
    sp.set_shadows(True)
    assert sp.shadow_field().shape == (48, 48)
    assert sp.render_rgba().shape == (120, 160, 4)


def test_the_field_follows_its_inputs_and_rests_otherwise(vf):
    import oracle
    W, H = 320, 200
    lut = viridis()
    h = heights(3)
    t = terrain(W, H, GRID, h, lut)
    t.set_shade_precision(0)
    t.set_shadows(True, **SCENE_PARAMS)

    def check(u, hh, what):
        t.render()
        got = t.read_rgba()
        rgba, vis = oracle.render_terrain(u, W, H, GRID, hh, lut, want_vis=True, nthreads=8)
        want, mask = shm.frame(rgba, vis, u, hh, GRID, lut, shm.field(u, hh, GRID, **SCENE_PARAMS))
        assert mask.any(), what
        assert_frame(got.reshape(H, W, 4), want, what)

    u = uniforms(W, H, sun=shm.sun_vector(*SCENE_SUN_DEG))
    t.set_uniforms(u)
    assert t.shadow_scans() == 0
    check(u, h, "first frame")
    assert t.shadow_scans() == 1
    for _ in range(3):                                        # a resting scene pays once
        t.render()
    t.read_rgba()
    assert t.shadow_scans() == 1
    t.set_uniforms(uniforms(W, H, cam="fill", sun=shm.sun_vector(*SCENE_SUN_DEG)))   # the camera alone: no new field
    t.render()
    assert t.shadow_scans() == 1
    u2 = uniforms(W, H, sun=shm.sun_vector(70.0, 200.0))
    t.set_uniforms(u2)
    check(u2, h, "new sun")
    assert t.shadow_scans() == 2
    u3 = uniforms(W, H, sun=shm.sun_vector(70.0, 200.0), exag=1.6)
    t.set_uniforms(u3)
    check(u3, h, "new exaggeration")
    assert t.shadow_scans() == 3
    h2 = heights(9)
    t.set_height(h2)
    check(u3, h2, "new heights")
    assert t.shadow_scans() == 4
    t.set_shadows(True, strength=0.5, softness=SCENE_PARAMS["softness"], bias=SCENE_PARAMS["bias"])
    t.render()
    assert t.shadow_scans() == 5
    ms = t.shadow_stage(3)
    assert ms[0] > 0 and ms[1] > 0 and t.shadow_scans() == 5  # (diagnostic launches are not the handle's)
    t.close()


def test_refusals_change_nothing(vf):
    from vulkan_forge_amd import cabi
    W, H = 128, 128
    h = heights(2, (32, 32))
    s = scene(vf, W, H, h)
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.set_shadows(True)
    s.set_shard(0, 1, 64)
    before = s.render_rgba().copy()
    t = terrain(W, H, 32, h)
    t.set_uniforms(uniforms(W, H))
    t.set_tile_shard(0, 2)
    assert t.lib.vf_terrain_set_shadows(t.t, 1, 0.7, 0.02, 0.002) == cabi.VF_ERR_INVALID
    assert "whole-frame handle" in t.lib.vf_last_error().decode()
    t.close()
    for bad in ((1.5, 0.02, 0.002), (0.7, 0.0, 0.002), (0.7, 0.02, -1.0), (float("nan"), 0.02, 0.002), (0.7, float("inf"), 0.002)):
        t = terrain(W, H, 32, h)
        assert t.lib.vf_terrain_set_shadows(t.t, 1, *bad) == cabi.VF_ERR_INVALID
        t.close()
    assert np.array_equal(s.render_rgba(), before)            # (the refused enable left the scene unshadowed)
    s.set_sun(*SCENE_SUN_DEG)
    s.set_shadows(True, **SCENE_PARAMS)
    shadowed = s.render_rgba().copy()
    with pytest.raises(RuntimeError, match="render_batch on a handle with shadows enabled"):
        s.render_batch([CAMERAS["default"], CAMERAS["fill"]])
    with pytest.raises(RuntimeError, match="shadows enabled"):
        s.set_shard(0, 2, 64)
    assert np.array_equal(s.render_rgba(), shadowed)
