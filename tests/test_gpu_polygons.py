"""Polygon overlays on the GPU (vf_overlay.h, k_pg_* and the fill walk of k_ov_composite) equal the CPU model (tests/polygon_model)
applied to the same handle's frame drawn without them, bit for bit -- every read-back path, batches of poses, near-plane crossings,
screen-covering fills, rings off every screen edge, vertices on pixel-centre rows, a 200 000-vertex ring, and a bin past the sort cap."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from support import vf  # noqa: F401
import polygon_model as pm
from overlay_scenes import CAMERAS, GRID, apply, heights, scene


def blob(rng, c, r, n, y):
    """a wobbly ring of n vertices around world (c[0], c[1]) in the x-z plane at height y"""
    a = np.sort(rng.uniform(0, 2 * np.pi, n))
    rr = r * rng.uniform(0.6, 1.0, n)
    return np.column_stack([c[0] + rr * np.cos(a), np.full(n, y), c[1] + rr * np.sin(a)]).astype(np.float32)


def polygons(rng, n, spread=1.6):
    polys = []
    for k in range(n):
        c = rng.uniform(-spread, spread, 2)
        r = rng.uniform(0.03, 0.35)
        y = rng.uniform(0.0, 0.3)
        outer = blob(rng, c, r, int(rng.integers(3, 40)), y)
        if k % 3 == 0:                                        # a donut
            polys.append([outer, blob(rng, c, 0.4 * r, int(rng.integers(3, 16)), y)])
        elif k % 3 == 1:                                      # a two-part multipolygon
            polys.append([outer, blob(rng, c + rng.uniform(-0.5, 0.5, 2), 0.5 * r, int(rng.integers(3, 12)), y)])
        else:
            polys.append(outer)
    return polys


def workload(seed=11, npoly=240, npts=3000, npaths=600):
    """(method, args, kwargs) calls: polygon layers interleaved with point and line layers; draped and not; fill only, outline only,
    fill + outline, per-feature colours; a long ring across the whole terrain and through the "near" camera"""
    rng = np.random.default_rng(seed)
    calls = []
    xyz = np.column_stack([rng.uniform(-1.6, 1.6, npts), rng.uniform(-0.2, 0.6, npts), rng.uniform(-1.6, 1.6, npts)]).astype(np.float32)
    calls.append(("add_points", (xyz,), dict(size_px=6.0, rgba=(240, 30, 30, 200))))
    P = polygons(rng, npoly)
    q = npoly // 4
    calls.append(("add_polygons", (P[:q],), dict(fill_rgba=(30, 120, 250, 140))))
    calls.append(("add_polygons", (P[q:2 * q],), dict(fill_rgba=rng.integers(0, 256, (q, 4), dtype=np.uint8), line_rgba=(10, 10, 10, 255),
                                                    line_width_px=1.0, drape=True)))
    paths = []
    for _ in range(npaths):
        m = int(rng.integers(2, 8))
        start = rng.uniform(-1.6, 1.6, 3) * [1, 0.2, 1]
        paths.append((start + np.cumsum(rng.normal(0, 0.08, (m, 3)) * [1, 0.2, 1], axis=0)).astype(np.float32))
    calls.append(("add_lines", (paths,), dict(width_px=2.0, rgba=(250, 250, 0, 255), cap="round")))
    big = [np.array([[-1.5, 0.3, -1.5], [1.5, 0.3, -1.2], [1.5, 0.5, 1.5], [0.2, 0.6, 0.1], [-1.5, 0.1, 1.5]], np.float32),
           np.array([[-0.5, 0.3, -0.5], [0.5, 0.3, -0.5], [0.0, 0.3, 0.6]], np.float32)]
    calls.append(("add_polygons", ([big] + P[2 * q:3 * q],), dict(fill_rgba=(200, 60, 220, 90), line_rgba=(255, 255, 255, 180), line_width_px=3.0)))
    calls.append(("add_polygons", (P[3 * q:],), dict(fill_rgba=None, line_rgba=(0, 255, 120, 255), line_width_px=2.0, drape=True)))
    return calls


def check(got, want, base):
    assert not np.array_equal(want, base)
    diff = (got != want).any(axis=2)
    assert not diff.any(), f"{int(diff.sum())} pixels differ from the model, first at {np.argwhere(diff)[:4].tolist()}"


@pytest.mark.parametrize("size", [(1920, 1080), (257, 131)])
@pytest.mark.parametrize("cam", list(CAMERAS))
def test_frames_equal_the_model(vf, size, cam):
    W, H = size
    h = heights()
    s = scene(vf, W, H, h, cam)
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    L = apply(vf, s, workload(), pm.Layers())
    got = s.render_rgba()
    check(got, pm.composite(base, u, h, GRID, L), base)
    assert np.array_equal(s.render_rgba(), got)               # (again: the pass leaves its counters and boxes as it found them)


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
    L = apply(vf, s, workload(3, 120, 800, 200), pm.Layers())
    frames = s.render_batch(poses)
    for k, p in enumerate(poses):
        assert np.array_equal(frames[k], pm.composite(bases[k], us[k], h, GRID, L)), f"pose {k}"
        s.set_camera_look_at(*p)
        assert np.array_equal(s.render_rgba(), frames[k]), f"pose {k}: batch != single render"
    s.render_png(str(tmp_path / "p.png"))
    png = np.asarray(Image.open(tmp_path / "p.png").convert("RGBA"))
    assert np.array_equal(png, pm.composite(bases[-1], us[-1], h, GRID, L))


@pytest.mark.parametrize("cam", ["fill", "near"])
def test_screen_covering_fill_and_rings_off_every_edge(vf, cam):
    W, H = 480, 272
    h = heights(6)
    s = scene(vf, W, H, h, cam)
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    rng = np.random.default_rng(4)
    cover = [np.array([[-40, 0.1, -40], [40, 0.1, -40], [40, 0.1, 40], [-40, 0.1, 40]], np.float32),     # all of the screen ...
             blob(rng, (0.1, 0.2), 0.4, 50, 0.2)]                                                          # ... but a hole
    across = [np.array([[-6, 0.2, -0.3], [6, 0.25, -0.2], [6, 0.2, 0.1], [-6, 0.3, 0.0]], np.float32),     # off the left and right edges
              np.array([[-0.3, 0.2, -6], [-0.1, 0.1, 6], [0.2, 0.2, 6], [0.1, 0.3, -6]], np.float32)]      # off the top and bottom edges
    calls = [("add_polygons", ([cover],), dict(fill_rgba=(20, 200, 90, 120))),
             ("add_polygons", (across,), dict(fill_rgba=(250, 90, 20, 200), line_rgba=(0, 0, 0, 255), line_width_px=2.0))]
    L = apply(vf, s, calls, pm.Layers())
    check(s.render_rgba(), pm.composite(base, u, h, GRID, L), base)


def test_vertices_on_pixel_centre_rows_and_horizontal_edges(vf, luts):
    from vulkan_forge_amd import cabi
    W, H = 256, 128
    h = heights(3)
    t = cabi.Terrain(W, H, 64, luts["viridis"])
    try:
        t.set_height(h)
        s = scene(vf, W, H, h)                                # (its uniforms, with an exact orthographic view / projection)
        u = s.debug_uniforms_f32().copy()
        u[0:16] = np.eye(4, dtype=np.float32).reshape(16)
        proj = np.zeros(16, np.float32)
        proj[0], proj[5], proj[14], proj[15] = 1.0, 1.0, 0.5, 1.0
        u[16:32] = proj
        t.set_uniforms(u)
        t.render()
        base = t.read_rgba().reshape(H, W, 4)

        def wp(sx, sy):                                       # screen (sx, sy) -> world, exact: screen = (128 (1 + x), 64 (1 - y))
            return [sx / 128.0 - 1.0, 1.0 - sy / 64.0, 0.0]
        rings = [np.array([wp(10.5, 10.5), wp(100.5, 10.5), wp(100.5, 60.5), wp(60.5, 30.5), wp(10.5, 60.5)], np.float32),
                 np.array([wp(120.5, 20.5), wp(200.25, 20.5), wp(240.5, 100.5), wp(150.5, 100.5), wp(150.5, 70.5), wp(130.5, 70.5)], np.float32),
                 np.array([wp(30.5, 80.5), wp(90.5, 80.5), wp(90.5, 120.5), wp(30.5, 120.5)], np.float32),
                 np.array([wp(40.5, 90.5), wp(80.5, 90.5), wp(80.5, 110.5), wp(40.5, 110.5)], np.float32)]
        coords, ro, fo = vf.pack_polygons([rings[0], rings[1], [rings[2], rings[3]]])
        t.add_polygons(coords, ro, fo, fill_rgba=(255, 255, 255, 200), line_rgba=None)
        t.render()
        got = t.read_rgba().reshape(H, W, 4)
        L = pm.Layers().polygons([rings[0], rings[1], [rings[2], rings[3]]], fill_rgba=(255, 255, 255, 200))
        check(got, pm.composite(base, u, h, 64, L), base)
    finally:
        t.close()


def test_a_200k_vertex_ring(vf):
    W, H = 1920, 1080
    h = heights(9)
    s = scene(vf, W, H, h, "fill")
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    n = 200_000
    a = np.linspace(0, 2 * np.pi, n, endpoint=False)
    r = 1.35 + 0.12 * np.sin(37 * a) + 0.05 * np.sin(1013 * a)
    ring = np.column_stack([r * np.cos(a), np.full(n, 0.2), r * np.sin(a)]).astype(np.float32)
    L = apply(vf, s, [("add_polygons", ([ring],), dict(fill_rgba=(60, 60, 255, 170), line_rgba=(255, 255, 255, 255)))], pm.Layers())
    check(s.render_rgba(), pm.composite(base, u, h, GRID, L), base)


def test_more_than_4096_primitives_in_one_bin(vf):
    W, H = 96, 80
    h = heights(2, (64, 64))
    s = scene(vf, W, H, h, "fill")
    base = s.render_rgba()
    u = s.debug_uniforms_f32()
    view, proj = u[0:16].reshape(4, 4).T.astype(np.float64), u[16:32].reshape(4, 4).T.astype(np.float64)
    inv = np.linalg.inv(proj @ view)
    o = proj @ view @ np.array([0.0, 0.0, 0.0, 1.0])
    rng = np.random.default_rng(12)
    polys = []
    for _ in range(1500):                                     # triangles in the bin at pixels (32..47, 32..47): 1 + 6 records each
        sx, sy = rng.uniform(33.0, 46.0, 3), rng.uniform(33.0, 46.0, 3)
        ndc = np.column_stack([sx / (W / 2) - 1.0, 1.0 - sy / (H / 2), np.full(3, o[2] / o[3]), np.ones(3)])
        p = ndc @ inv.T
        polys.append((p[:, :3] / p[:, 3:4]).astype(np.float32))
    cols = rng.integers(0, 256, (1500, 4), dtype=np.uint8)
    cols[:, 3] = rng.integers(40, 256, 1500)
    L = apply(vf, s, [("add_polygons", (polys,), dict(fill_rgba=cols))], pm.Layers())
    check(s.render_rgba(), pm.composite(base, u, h, GRID, L), base)


def test_outline_only_equals_add_lines_of_the_closed_rings(vf):
    W, H = 400, 240
    h = heights(4)
    rng = np.random.default_rng(8)
    P = polygons(rng, 60)
    a = scene(vf, W, H, h)
    a.add_polygons(P, fill_rgba=None, line_rgba=(255, 40, 40, 200), line_width_px=2.5, drape=True)
    b = scene(vf, W, H, h)
    coords, rings, feats = vf.pack_polygons(P)
    closed = [np.vstack([coords[rings[r]:rings[r + 1]], coords[rings[r]:rings[r] + 1]]) for r in range(len(rings) - 1)]
    b.add_lines(closed, width_px=2.5, rgba=(255, 40, 40, 200), cap="round", drape=True)
    assert np.array_equal(a.render_rgba(), b.render_rgba())


def test_clear_overlays_restores_a_plain_handle_and_shards_refuse(vf):
    W, H = 320, 200
    h = heights(4)
    plain = scene(vf, W, H, h).render_rgba()
    s = scene(vf, W, H, h)
    apply(vf, s, workload(1, 60, 300, 80), pm.Layers())
    assert not np.array_equal(s.render_rgba(), plain)
    s.clear_overlays()
    assert np.array_equal(s.render_rgba(), plain)
    tri = np.array([[0, 0.2, 0], [0.5, 0.2, 0], [0, 0.2, 0.5]], np.float32)
    assert s.add_polygons([tri]) == 0                         # layer ids count again from zero
    assert not np.array_equal(s.render_rgba(), plain)
    with pytest.raises(RuntimeError, match="overlays"):
        s.set_shard(0, 2, 64)
    t = vf.Scene(64, 128, grid=32)
    t.set_shard(1, 2, 64)
    with pytest.raises(RuntimeError, match="whole-frame"):
        t.add_polygons([tri])
    with pytest.raises(ValueError, match="cannot both be None"):
        s.add_polygons([tri], fill_rgba=None)
