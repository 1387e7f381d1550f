"""Overlays on the GPU (vf_overlay.h) equal the CPU model (tests/overlay_model) applied to the same handle's frame drawn without them,
bit for bit -- every read-back path, batches of poses, partial bins, near-plane crossings, and a million points in one bin."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from support import vf  # noqa: F401
import overlay_model as om
from overlay_scenes import CAMERAS, GRID, apply, heights, scene


def workload(seed=11, npts=10_000, npaths=2_000):
    """(list of (method, args, kwargs)) -- mixed points and polylines, draped and not, every shape and cap"""
    rng = np.random.default_rng(seed)
    calls = []
    for k, (shape, drape) in enumerate([("circle", False), ("square", True), ("circle", True), ("square", False)]):
        n = npts // 4
        xyz = np.column_stack([rng.uniform(-1.6, 1.6, n), rng.uniform(-0.2, 0.6, n) if not drape else rng.uniform(0.0, 0.1, n),
                               rng.uniform(-1.6, 1.6, n)]).astype(np.float32)
        if k == 0:
            sizes = rng.uniform(0.5, 12.0, n).astype(np.float32)
            cols = rng.integers(0, 256, (n, 4), dtype=np.uint8)
            calls.append(("add_points", (xyz,), dict(size_px=sizes, rgba=cols, shape=shape, drape=drape)))
        else:
            calls.append(("add_points", (xyz,), dict(size_px=float(2 + 3 * k), rgba=(int(40 * k), 200, 90, 100 + 40 * k), shape=shape, drape=drape)))
    for k, (cap, drape) in enumerate([("round", False), ("butt", True), ("square", False), ("round", True)]):
        paths = []
        for _ in range(npaths // 4):
            m = int(rng.integers(2, 8))
            start = rng.uniform(-1.6, 1.6, 3) * [1, 0.2, 1]
            steps = rng.normal(0, 0.08, (m, 3)) * [1, 0.2, 1]
            paths.append((start + np.cumsum(steps, axis=0)).astype(np.float32))
        if k == 0:                                            # long lines across the whole terrain (and through the "near" camera)
            paths += [np.array([[-1.5, 0.3, -1.5], [1.5, 0.3, 1.5]], np.float32), np.array([[1.5, 0.5, -1.5], [-1.5, 0.1, 1.5], [0.2, 0.6, 0.1]], np.float32)]
        calls.append(("add_lines", (paths,), dict(width_px=float(1 + 2 * k), rgba=(255 - 50 * k, 40 * k, 120, 255 if k % 2 else 150), cap=cap, drape=drape)))
    return calls


@pytest.mark.parametrize("size", [(1920, 1080), (257, 131)])
@pytest.mark.parametrize("cam", list(CAMERAS))
def test_frames_equal_the_model(vf, size, cam):
    W, H = size
    h = heights()
    s = scene(vf, W, H, h, cam)
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    L = apply(vf, s, workload(), om.Layers())
    got = s.render_rgba()
    want = om.composite(base, u, h, GRID, L)
    assert not np.array_equal(want, base)
    diff = (got != want).any(axis=2)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the model, first at {np.argwhere(diff)[:4].tolist()}"
    assert np.array_equal(s.render_rgba(), got)               # (again: the pass leaves its counters as it found them)


def test_png_and_batch_equal_the_model(vf, tmp_path):
    from PIL import Image
    W, H = 640, 360
    h = heights(5)
    s = scene(vf, W, H, h)
    poses = [((3.0 * np.cos(a), 2.0, 3.0 * np.sin(a)), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0) for a in np.linspace(0, 2 * np.pi, 5)[:4]]
    bases, us = [], []
    for p in poses:
        s.set_camera_look_at(*p)
        bases.append(s.render_rgba())
        us.append(s.debug_uniforms_f32())
    L = apply(vf, s, workload(3, 4000, 800), om.Layers())
    frames = s.render_batch(poses)
    for k, p in enumerate(poses):
        want = om.composite(bases[k], us[k], h, GRID, L)
        assert np.array_equal(frames[k], want), f"pose {k}"
        s.set_camera_look_at(*p)
        assert np.array_equal(s.render_rgba(), frames[k]), f"pose {k}: batch != single render"
    s.render_png(str(tmp_path / "o.png"))
    png = np.asarray(Image.open(tmp_path / "o.png").convert("RGBA"))
    assert np.array_equal(png, om.composite(bases[-1], us[-1], h, GRID, L))


def test_a_million_points_in_one_bin_keep_their_order(vf):
    W, H = 96, 80
    h = heights(2, (64, 64))
    s = scene(vf, W, H, h, "fill")
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    # world points that project into the 16 x 16 bin at pixels (32..47, 32..47): solve on the CPU model's own transform
    view, proj = u[0:16].reshape(4, 4).T, u[16:32].reshape(4, 4).T
    inv = np.linalg.inv(proj.astype(np.float64) @ view.astype(np.float64))
    rng = np.random.default_rng(9)
    n = 1_000_000
    sx, sy = rng.uniform(36.0, 44.0, n), rng.uniform(36.0, 44.0, n)
    o = proj.astype(np.float64) @ view.astype(np.float64) @ np.array([0.0, 0.0, 0.0, 1.0])    # the depth of the terrain's centre
    ndc = np.column_stack([sx / (W / 2) - 1.0, 1.0 - sy / (H / 2), np.full(n, o[2] / o[3]), np.ones(n)])
    p = ndc @ inv.T
    xyz = (p[:, :3] / p[:, 3:4]).astype(np.float32)
    cols = rng.integers(0, 256, (n, 4), dtype=np.uint8)
    cols[:, 3] = rng.integers(128, 256, n)
    sizes = rng.uniform(1.0, 3.0, n).astype(np.float32)
    s.add_points(xyz, size_px=sizes, rgba=cols, shape="square")
    got = s.render_rgba()
    want = om.composite(base, u, h, GRID, om.Layers().points(xyz, size_px=sizes, rgba=cols, shape="square"))
    assert not np.array_equal(want, base)
    assert np.array_equal(got, want)


def test_clear_overlays_restores_a_plain_handle(vf):
    W, H = 320, 200
    h = heights(4)
    plain = scene(vf, W, H, h).render_rgba()
    s = scene(vf, W, H, h)
    apply(vf, s, workload(1, 2000, 300), om.Layers())
    assert not np.array_equal(s.render_rgba(), plain)
    s.clear_overlays()
    assert np.array_equal(s.render_rgba(), plain)
    assert s.add_points(np.zeros((1, 3), np.float32)) == 0    # layer ids count again from zero
    assert s.add_lines([np.eye(3, dtype=np.float32)]) == 1


def test_visibility_read_back_ignores_overlays(vf):
    W, H = 160, 120
    h = heights(8)
    plain = scene(vf, W, H, h)
    plain.render_rgba()
    vis = plain.debug_visibility()
    s = scene(vf, W, H, h)
    apply(vf, s, workload(2, 500, 100), om.Layers())
    s.render_rgba()
    assert np.array_equal(s.debug_visibility(), vis)


def test_errors(vf):
    s = vf.Scene(64, 64, grid=32)
    pts = np.zeros((2, 3), np.float32)
    with pytest.raises(TypeError):
        s.add_points(pts.astype(np.int32))
    with pytest.raises(ValueError):
        s.add_points(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError):
        s.add_points(pts, shape="hexagon")
    with pytest.raises(ValueError):
        s.add_lines([np.eye(3, dtype=np.float32)], cap="arrow")
    with pytest.raises(TypeError):
        s.add_points(pts, rgba=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError):
        s.add_lines([np.array([[0, 0, 0], [np.inf, 0, 0]], np.float32)])
    assert s.add_points(np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32)) == 0     # a non-finite point is dropped, not an error
    with pytest.raises(RuntimeError, match="overlays"):
        s.set_shard(0, 2, 64)
    t = vf.Scene(64, 128, grid=32)
    t.set_shard(1, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame"):
        t.add_points(pts)
