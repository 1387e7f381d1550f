"""Geometry buffers on the GPU equal the CPU model (tests/gbuffer_model) run on the oracle's visibility of the same
frame, bit for bit -- both shade precisions, three cameras, every subset of planes, pick, the C-ABI and device destinations -- and
leave the handle's frames, timing and output as they were."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import support
import gbuffer_model as gbm
from overlay_scenes import CAMERAS, GRID, heights, scene
from support import bits, vf  # noqa: F401

PLANES = ("depth", "position", "normal", "primitive")


def oracle_vis(u, W, H, h):
    import oracle
    return oracle.render_terrain(u, W, H, GRID, h, np.zeros(1024, np.uint8), want_vis=True, nthreads=8)[1]


def assert_planes_equal(got, want, what=""):
    for k in want:
        d = bits(got[k]) != bits(want[k])
        assert not d.any(), f"{what}{k}: {int(d.sum())} words differ, first at {np.argwhere(d)[:4].tolist()}"


@pytest.mark.parametrize("size", [(1920, 1080), (257, 131)])
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_planes_equal_the_model(vf, size, cam):
    W, H = size
    h = heights()
    got = {}
    for precision in ("fast", "exact"):
        s = scene(vf, W, H, h, cam, precision)
        g = s.render_gbuffer()
        assert set(g) == set(PLANES)
        assert g["depth"].shape == (H, W) and g["position"].shape == (H, W, 3) and g["normal"].shape == (H, W, 3) and g["primitive"].shape == (H, W)
        assert g["depth"].dtype == np.float32 and g["primitive"].dtype == np.uint32
        assert np.array_equal(g["primitive"], s.debug_visibility())
        got[precision] = g
        u = s.debug_uniforms_f32()
    vis = oracle_vis(u, W, H, h)
    depth, position, normal = gbm.planes(vis, u, h, GRID)
    want = {"depth": depth, "position": position, "normal": normal, "primitive": vis}
    assert (vis != 0).any()
    for precision in got:
        assert_planes_equal(got[precision], want, f"{precision} ")
    assert_planes_equal(got["fast"], got["exact"], "fast against exact: ")


def test_every_subset_of_planes_and_render_depth(vf):
    W, H = 257, 131
    s = scene(vf, W, H, heights(), "near")
    full = s.render_gbuffer()
    for r in range(1, 5):
        for names in itertools.combinations(PLANES, r):
            g = s.render_gbuffer(names[::-1])
            assert tuple(g) == names[::-1]
            assert_planes_equal(g, {k: full[k] for k in names}, f"{names} ")
    assert np.array_equal(bits(s.render_depth()), bits(full["depth"]))
    sp = vf.TerrainSpike(160, 120, grid=48)
    gs = sp.render_gbuffer(["depth", "primitive"])
    assert np.array_equal(gs["primitive"], sp.debug_visibility()) and np.array_equal(np.isinf(gs["depth"]), gs["primitive"] == 0)
    assert np.array_equal(bits(sp.render_depth()), bits(gs["depth"]))


@pytest.mark.parametrize("cam", ["default", "near"])
def test_pick_equals_the_planes(vf, cam):
    W, H = 1920, 1080
    s = scene(vf, W, H, heights(), cam)
    full = s.render_gbuffer()
    rng = np.random.default_rng(12)
    px = np.column_stack([rng.integers(0, W, 1000), rng.integers(0, H, 1000)])
    px = np.concatenate([px, [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]])
    got = s.pick(px)
    at = (px[:, 1], px[:, 0])
    assert got["depth"].shape == (1004,) and got["position"].shape == (1004, 3) and got["normal"].shape == (1004, 3) and got["primitive"].shape == (1004,)
    assert (got["primitive"] != 0).sum() > 20
    assert_planes_equal(got, {k: full[k][at] for k in PLANES}, "pick ")
    one = s.pick([[int(px[0, 0]), int(px[0, 1])]])
    assert_planes_equal(one, {k: full[k][at][:1] for k in PLANES}, "pick of one ")
    for bad in ([W, 0], [0, H], [-1, 5]):
        with pytest.raises(ValueError, match="outside"):
            s.pick(np.array([[1, 1], bad]))


def test_pick_out_of_frame_writes_nothing_through_the_c_abi():
    from vulkan_forge_amd import cabi
    t = cabi.Terrain(96, 64, 32, np.zeros(1024, np.uint8))
    import oracle
    t.set_uniforms(oracle.default_uniforms(oracle.KIND_SCENE, 96, 64))
    t.render()
    px = np.array([[3, 3], [96, 3]], np.int32)
    out = np.full((2, 8), 0xDEADBEEF, np.uint32)
    assert t.lib.vf_terrain_pick(t.t, px.ctypes.data, 2, out.ctypes.data) == cabi.VF_ERR_INVALID
    assert "outside" in t.lib.vf_last_error().decode()
    assert (out == 0xDEADBEEF).all()
    assert t.lib.vf_terrain_read_gbuffer(t.t, None, None, None, None) == cabi.VF_ERR_INVALID
    t.close()


def overlay_calls(rng):
    n = 3000
    pts = np.column_stack([rng.uniform(-1.5, 1.5, n), rng.uniform(0.0, 0.1, n), rng.uniform(-1.5, 1.5, n)]).astype(np.float32)
    paths = [(rng.uniform(-1.4, 1.4, 3) * [1, 0.03, 1] + np.cumsum(rng.normal(0, 0.08, (5, 3)) * [1, 0.03, 1], axis=0)).astype(np.float32) for _ in range(200)]
    poly = [np.array([[-0.6, 0.05, -0.6], [0.7, 0.05, -0.5], [0.1, 0.05, 0.8]], np.float32)]
    return pts, paths, poly


def test_nothing_else_moves(vf):
    W, H = 640, 400
    h = heights(5)
    plain = scene(vf, W, H, h)
    want = plain.render_gbuffer()
    s = scene(vf, W, H, h)
    pts, paths, poly = overlay_calls(np.random.default_rng(2))
    s.add_points(pts, size_px=5.0, rgba=(255, 0, 0, 255), drape=True, occlude=True)
    s.add_lines(paths, width_px=3.0, rgba=(0, 255, 0, 200), drape=True)
    s.add_polygons(poly, fill_rgba=(0, 90, 255, 160), line_rgba=(0, 0, 0, 255), drape=True)
    s.add_lines(paths[:50], width_px=2.0, rgba=(255, 255, 0, 255), drape=True, occlude=True, depth_bias=0.02)
    for obj in (plain, s):
        before = obj.render_rgba().copy()
        obj.enable_timing(True)
        obj.render_rgba()
        frames = obj.last_timings()["frames"]
        g = obj.render_gbuffer()
        obj.pick([[5, 5], [W // 2, H // 2]])
        obj.render_depth()
        assert obj.last_timings()["frames"] == frames
        obj.enable_timing(False)
        assert_planes_equal(g, want)                          # overlays in the frame, none in the planes
        assert np.array_equal(obj.render_rgba(), before)
    assert (s.render_rgba() != plain.render_rgba()).any()
    # the planes follow the camera like render_rgba does
    s.set_camera_look_at(*CAMERAS["fill"])
    moved = s.render_gbuffer(["primitive"])["primitive"]
    assert np.array_equal(moved, s.debug_visibility()) and not np.array_equal(moved, want["primitive"])


def test_sharded_handles_are_refused(vf):
    from vulkan_forge_amd import cabi
    s = scene(vf, 128, 128, heights(2, (32, 32)))
    s.set_shard(0, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.render_gbuffer()
    with pytest.raises(RuntimeError, match="whole-frame handle"):
        s.pick([[1, 1]])
    t = cabi.Terrain(128, 128, 32, np.zeros(1024, np.uint8))
    import oracle
    t.set_uniforms(oracle.default_uniforms(oracle.KIND_SCENE, 128, 128))
    t.set_tile_shard(0, 2)
    out = np.zeros((128, 128), np.float32)
    assert t.lib.vf_terrain_read_gbuffer(t.t, out.ctypes.data, None, None, None) == cabi.VF_ERR_INVALID
    t.close()


def cabi_scene(W, H, h, cam):
    import oracle
    from vulkan_forge_amd import cabi
    t = cabi.Terrain(W, H, GRID, np.zeros(1024, np.uint8))
    t.set_height(h)
    u = oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam])
    t.set_uniforms(u)
    return t, u


def test_the_planes_belong_to_the_frame_that_was_rendered():
    """vf_terrain_render without waiting, new uniforms set, then the read: the rule of vf_terrain_read_visibility"""
    import oracle
    W, H = 640, 360
    h = heights(3)
    t, u = cabi_scene(W, H, h, "default")
    before = t.read_gbuffer(["primitive"])["primitive"]       # before the first render: the current uniforms
    t.render()                                                # (queued, not waited for)
    t.set_uniforms(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["fill"]))
    g = t.read_gbuffer()
    vis = oracle_vis(u, W, H, h)
    depth, position, normal = gbm.planes(vis, u, h, GRID)
    assert_planes_equal(g, {"depth": depth, "position": position, "normal": normal, "primitive": vis})
    assert np.array_equal(before, vis)
    assert np.array_equal(t.read_visibility(), vis)
    got = t.pick(np.array([[W // 2, H // 2], [10, 300]]))
    assert_planes_equal(got, {k: g[k][[H // 2, 300], [W // 2, 10]] for k in PLANES})
    t.close()


def test_device_destinations_on_a_stream_of_the_callers():
    """vf_terrain_gbuffer_device into torch tensors on a torch stream equals the host read (a fresh process: torch is imported before
    the library there, one HIP runtime per process)"""
    support.run_check("gbuffer_torch_check.py", "GBUFFER TORCH OK")
