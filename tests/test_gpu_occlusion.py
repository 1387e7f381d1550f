"""Occluding overlay layers on the GPU equal the CPU model (tests/occlusion_model) applied to the same handle's frame
drawn without overlays and the oracle's visibility of it, bit for bit -- both shade precisions, three cameras, layers that mix
occluding, plain and polygon layers, every read-back path, frames in flight, and switching occlusion between frames."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from support import ridge, vf  # noqa: F401
import occlusion_model as ocm
from overlay_scenes import GRID, apply, heights, scene

RIDGE = ((0.0, 1.0, 3.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 100.0)     # from in front of ridge(), over its crest


def oracle_vis(u, W, H, h):
    import oracle
    lut = np.zeros(1024, np.uint8)
    return oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True, nthreads=8)[1]


def workload(seed=11, npts=8000, npaths=1200):
    """(method, args, kwargs) calls: point, line and polygon layers; every other point / line layer occludes"""
    rng = np.random.default_rng(seed)
    calls = []
    for k, (shape, drape) in enumerate([("circle", True), ("square", True), ("circle", False), ("square", True)]):
        n = npts // 4
        xyz = np.column_stack([rng.uniform(-1.6, 1.6, n), rng.uniform(-0.05, 0.1, n) if drape else rng.uniform(-0.2, 0.6, n),
                               rng.uniform(-1.6, 1.6, n)]).astype(np.float32)
        kw = dict(size_px=float(2 + 3 * k), rgba=(int(40 * k), 200, 90, 120 + 40 * k), shape=shape, drape=drape, occlude=k % 2 == 0)
        if k == 0:
            kw.update(size_px=rng.uniform(0.5, 12.0, n).astype(np.float32), rgba=rng.integers(0, 256, (n, 4), dtype=np.uint8), depth_bias=0.0)
        calls.append(("add_points", (xyz,), kw))
    for k, (cap, drape) in enumerate([("round", True), ("butt", True), ("square", False)]):
        paths = []
        for _ in range(npaths // 3):
            m = int(rng.integers(2, 8))
            start = rng.uniform(-1.6, 1.6, 3) * [1, 0.05, 1]
            paths.append((start + np.cumsum(rng.normal(0, 0.08, (m, 3)) * [1, 0.05, 1], axis=0)).astype(np.float32))
        if k == 0:                                            # long lines across the terrain and through the "near" camera
            paths += [np.array([[-1.5, 0.3, -1.5], [1.5, 0.3, 1.5]], np.float32), np.array([[1.5, 0.5, -1.5], [-1.5, 0.1, 1.5], [0.2, 0.6, 0.1]], np.float32)]
        calls.append(("add_lines", (paths,), dict(width_px=float(1 + 2 * k), rgba=(255 - 50 * k, 40 * k, 120, 255 if k % 2 else 150), cap=cap,
                                                  drape=drape, occlude=k != 1, depth_bias=(0.05, 0.0, 1e-3)[k])))
    calls.append(("add_polygons", ([np.array([[-0.6, 0.05, -0.6], [0.7, 0.05, -0.5], [0.1, 0.05, 0.8]], np.float32)],),
                  dict(fill_rgba=(0, 90, 255, 120), line_rgba=(0, 0, 0, 255), line_width_px=2.0, drape=True)))
    return calls


@pytest.mark.parametrize("precision", ["fast", "exact"])
@pytest.mark.parametrize("size", [(1920, 1080), (257, 131)])
@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_frames_equal_the_model(vf, size, cam, precision):
    W, H = size
    h = heights()
    s = scene(vf, W, H, h, cam, precision)
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    vis = oracle_vis(u, W, H, h)
    L = apply(vf, s, workload(), ocm.Layers())
    got = s.render_rgba()
    want = ocm.composite(base, vis, u, h, GRID, L)
    assert not np.array_equal(want, ocm.pm.composite(base, u, h, GRID, L))    # (occlusion changes the frame)
    diff = (got != want).any(axis=2)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the model, first at {np.argwhere(diff)[:4].tolist()}"
    assert np.array_equal(s.render_rgba(), got)


def test_the_ridge_hides_what_lies_behind_it(vf):
    W, H = 640, 400
    h = ridge()
    s = scene(vf, W, H, h)
    s.set_camera_look_at(*RIDGE)
    base = s.render_rgba()
    xs = np.linspace(-1.2, 1.2, 25, dtype=np.float32)
    behind = np.column_stack([xs, np.full(25, 0.02, np.float32), np.full(25, -0.9, np.float32)])
    front = behind * np.float32([1, 1, -1])
    s.add_points(behind, size_px=6, rgba=(255, 0, 0, 255), drape=True, occlude=True)
    s.add_lines([behind], width_px=5, rgba=(255, 0, 0, 255), drape=True, occlude=True)
    assert np.array_equal(s.render_rgba(), base)              # everything behind the ridge: not a pixel changes
    s.add_points(front, size_px=6, rgba=(255, 0, 0, 255), drape=True, occlude=True)
    assert (s.render_rgba() != base).any(axis=2).sum() > 300  # what stands in front of it is drawn


def test_png_batch_streaming_and_toggling_equal_the_model(vf, tmp_path):
    from PIL import Image
    W, H = 640, 360
    h = heights(5)
    s = scene(vf, W, H, h)
    poses = [((3.0 * np.cos(a), 2.0, 3.0 * np.sin(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0) for a in np.linspace(0, 2 * np.pi, 5)[:4]]
    bases, us, viss = [], [], []
    for p in poses:
        s.set_camera_look_at(*p)
        bases.append(s.render_rgba())
        us.append(s.debug_uniforms_f32())
        viss.append(oracle_vis(us[-1], W, H, h))
    L = apply(vf, s, workload(3, 4000, 600), ocm.Layers())
    frames = s.render_batch(poses)                            # per-pose visibility
    for k in range(len(poses)):
        assert np.array_equal(frames[k], ocm.composite(bases[k], viss[k], us[k], h, GRID, L)), f"pose {k}"
    s.set_camera_look_at(*poses[-1])
    for _ in range(6):                                        # a caller that streams frames of a resting camera: frames in flight
        s.render_rgba()
    s.render_png(str(tmp_path / "o.png"))
    png = np.asarray(Image.open(tmp_path / "o.png").convert("RGBA"))
    assert np.array_equal(png, ocm.composite(bases[-1], viss[-1], us[-1], h, GRID, L))
    # occlusion switched per layer between frames: off for layer 0, on for layer 1 (points) with its own bias
    s.set_layer_occlusion(0, False)
    s.set_layer_occlusion(1, True, depth_bias=0.02)
    L.set_occlusion(0, False)
    L.set_occlusion(1, True, 0.02)
    assert np.array_equal(s.render_rgba(), ocm.composite(bases[-1], viss[-1], us[-1], h, GRID, L))


def test_clear_overlays_restores_a_plain_handle(vf):
    W, H = 320, 200
    h = heights(4)
    plain = scene(vf, W, H, h).render_rgba()
    s = scene(vf, W, H, h)
    apply(vf, s, workload(1, 2000, 300), ocm.Layers())
    assert not np.array_equal(s.render_rgba(), plain)
    s.clear_overlays()
    assert np.array_equal(s.render_rgba(), plain)
    assert np.array_equal(s.render_rgba(), plain)


def test_visibility_read_back_is_unchanged_by_occlusion(vf):
    W, H = 160, 120
    h = heights(8)
    plain = scene(vf, W, H, h)
    plain.render_rgba()
    vis = plain.debug_visibility()
    s = scene(vf, W, H, h)
    apply(vf, s, workload(2, 500, 90), ocm.Layers())
    s.render_rgba()
    assert np.array_equal(s.debug_visibility(), vis)


def test_set_layer_occlusion_refuses(vf):
    from vulkan_forge_amd import cabi
    s = scene(vf, 96, 64, heights(2, (32, 32)))
    s.add_points(np.zeros((2, 3), np.float32))
    s.add_polygons([np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)])
    with pytest.raises(RuntimeError, match="polygon"):
        s.set_layer_occlusion(1, True)
    with pytest.raises(RuntimeError, match="no overlay layer"):
        s.set_layer_occlusion(2, True)
    with pytest.raises(ValueError, match="depth_bias"):
        s.set_layer_occlusion(0, True, depth_bias=-1.0)
    s.set_layer_occlusion(0, True)
    lib = cabi.load()
    t = cabi.Terrain(64, 128, 32, np.zeros(1024, np.uint8))
    t.set_shard(1, 2, 64)
    assert lib.vf_terrain_set_layer_occlusion(t.t, 0, 1, 0.01) == cabi.VF_ERR_INVALID
    t.close()
