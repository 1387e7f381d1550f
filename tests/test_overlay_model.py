"""The overlay CPU model (tests/overlay_model) against the contract of DESIGN.md "Overlays": the model is what the GPU frames are
held to bit for bit (tests/test_gpu_overlays.py), so its own behaviour is pinned here on hand-checkable cases."""

import numpy as np
import pytest

import support  # noqa: F401  (the repository root and the model directories on sys.path)
import overlay_model as om

W = H = 64
BG = np.array([90, 60, 30, 255], np.uint8)


def ortho_uniforms(spacing=1.0, exag=1.0):
    """view = identity, proj: clip = (x, y, 0.5, 1): screen = (32 + 32 x, 32 - 32 y) on the 64 x 64 frame"""
    u = np.zeros(44, np.float32)
    u[0:16] = np.eye(4, dtype=np.float32).reshape(16)
    proj = np.zeros(16, np.float32)
    proj[0], proj[5], proj[14], proj[15] = 1.0, 1.0, 0.5, 1.0     # column-major: col 3 = (0, 0, 0.5, 1)
    u[16:32] = proj
    u[36], u[38] = spacing, exag
    return u


def world(sx, sy):
    return [(sx - 32.0) / 32.0, (32.0 - sy) / 32.0, 0.0]


def frame():
    return np.broadcast_to(BG, (H, W, 4)).copy()


TEX = np.zeros((1, 1), np.float32)


def run(layers, u=None):
    return om.composite(frame(), ortho_uniforms() if u is None else u, TEX, 2, layers)


def changed(a):
    return np.argwhere((a != frame()).any(axis=2))


def test_square_point_on_a_pixel_corner_replaces_exactly_a_4x4_block():
    out = run(om.Layers().points([world(20.0, 20.0)], size_px=4, rgba=(200, 10, 100, 255), shape="square"))
    ys, xs = changed(out).T
    assert sorted(set(ys.tolist())) == [18, 19, 20, 21] and sorted(set(xs.tolist())) == [18, 19, 20, 21] and len(ys) == 16
    assert (out[18:22, 18:22] == [200, 10, 100, 255]).all()


def test_transparent_and_offscreen_primitives_leave_the_frame_byte_identical():
    L = om.Layers()
    L.points([world(20, 20), world(40, 40)], size_px=9, rgba=(255, 0, 0, 0))
    L.lines([np.array([world(5, 5), world(50, 30), world(10, 60)], np.float32)], width_px=5, rgba=(0, 255, 0, 0))
    L.points([world(-40, 20), world(20, 200), world(1000, -1000)], size_px=30, rgba=(255, 255, 255, 255))
    L.lines([np.array([world(-100, 10), world(-20, 50)], np.float32)], width_px=8, rgba=(255, 255, 255, 255))
    behind = np.array([[0.0, 0.0, 0.0]], np.float32)
    u = ortho_uniforms()
    u[16 + 15] = -1.0                                         # w = -1: every vertex behind the camera
    assert np.array_equal(run(L), frame())
    assert np.array_equal(run(om.Layers().points(behind, size_px=20), u), frame())


def test_srgb_decode_then_encode_is_the_identity():
    assert all(om.encode(om.decode(b)) == b for b in range(256))


def test_a_translucent_polyline_blends_once_at_its_joints():
    col = (250, 250, 250, 128)
    path = np.array([world(10.5, 30.5), world(40.5, 30.5), world(40.5, 60.5)], np.float32)
    out = run(om.Layers().lines([path], width_px=6, rgba=col, cap="butt"))
    single = run(om.Layers().lines([path[:2]], width_px=6, rgba=col, cap="butt"))
    assert np.array_equal(out[30, 40], single[30, 20])        # the joint: covered by both segments and the disc, blended once
    assert np.array_equal(out[30, 20], single[30, 20])
    assert not np.array_equal(out[30, 40], frame()[30, 40])


def test_the_later_of_two_opaque_points_wins():
    a = (world(20, 20), (255, 0, 0, 255))
    b = (world(22, 20), (0, 0, 255, 255))
    ab = run(om.Layers().points([a[0]], size_px=8, rgba=a[1]).points([b[0]], size_px=8, rgba=b[1]))
    ba = run(om.Layers().points([b[0]], size_px=8, rgba=b[1]).points([a[0]], size_px=8, rgba=a[1]))
    assert list(ab[20, 21]) == [0, 0, 255, 255] and list(ba[20, 21]) == [255, 0, 0, 255]
    one = run(om.Layers().points(np.array([a[0], b[0]], np.float32), size_px=8, rgba=np.array([a[1], b[1]], np.uint8)))
    assert np.array_equal(one, ab)                            # features within a layer: input order


def test_caps_differ_exactly_where_the_formulas_say():
    seg = np.array([world(10.0, 20.5), world(30.0, 20.5)], np.float32)   # horizontal, on row 20's pixel centres, half width 2
    out = {cap: run(om.Layers().lines([seg], width_px=4, rgba=(255, 255, 255, 255), cap=cap)) for cap in ("butt", "square", "round")}
    white = [255, 255, 255, 255]
    # pixel (31, 20), centre 1.5 px beyond the end: butt sd = 1.5 (nothing); square sd = -0.5 and round sd = -0.5 (full)
    assert np.array_equal(out["butt"][20, 31], BG)
    assert list(out["square"][20, 31]) == white and list(out["round"][20, 31]) == white
    # pixel (31, 22), centre (1.5, 2) off the end: square sd = max(0, -0.5) = 0 (half), round sd = 2.5 - 2 = 0.5 (nothing)
    assert not np.array_equal(out["square"][22, 31], BG) and np.array_equal(out["round"][22, 31], BG)
    # inside the segment all three agree; butt never reaches past the ends
    assert np.array_equal(out["butt"][18:23, 10:30], out["square"][18:23, 10:30])
    assert np.array_equal(out["butt"][18:23, 10:30], out["round"][18:23, 10:30])
    assert np.array_equal(out["butt"][:, 30:], frame()[:, 30:]) and np.array_equal(out["butt"][:, :10], frame()[:, :10])


def test_drape_follows_the_vertex_stage_and_the_bc_diagonal():
    rng = np.random.default_rng(3)
    tex = rng.normal(size=(5, 7)).astype(np.float32)
    grid, step = 13, np.float32(0.25)                        # x_i = -1.5 + i / 4: exact in binary32
    u = ortho_uniforms()
    for i, j in [(0, 0), (3, 5), (12, 12), (7, 0), (11, 4)]:
        x, z = np.float32(-1.5) + np.float32(i) * step, np.float32(-1.5) + np.float32(j) * step
        assert om.drape(u, tex, grid, x, z) == om.vertex_height(tex, grid, i, j)
    i, j = 4, 6
    h = {k: np.float32(om.vertex_height(tex, grid, i + di, j + dj)) for k, (di, dj) in {"a": (0, 0), "b": (1, 0), "c": (0, 1), "d": (1, 1)}.items()}
    x0, z0 = np.float32(-1.5) + np.float32(i) * step, np.float32(-1.5) + np.float32(j) * step
    fx, fz = np.float32(0.25), np.float32(0.5)               # fx + fz <= 1: triangle (a, b, c)
    want = (h["a"] + fx * (h["b"] - h["a"])) + fz * (h["c"] - h["a"])
    assert om.drape(u, tex, grid, x0 + fx * step, z0 + fz * step) == np.float32(want)
    fx, fz = np.float32(0.75), np.float32(0.5)               # beyond the b-c diagonal: triangle (b, c, d)
    one = np.float32(1)
    want = (h["d"] + (one - fx) * (h["c"] - h["d"])) + (one - fz) * (h["b"] - h["d"])
    assert om.drape(u, tex, grid, x0 + fx * step, z0 + fz * step) == np.float32(want)
    # outside the grid: clamped to the edge
    assert om.drape(u, tex, grid, 9.0, -9.0) == om.vertex_height(tex, grid, 12, 0)


def test_a_draped_point_sits_on_the_surface_plus_its_offset():
    tex = np.full((2, 2), 0.25, np.float32)
    u = ortho_uniforms()                                      # y = h + offset goes straight to the screen row
    h = om.drape(u, tex, 5, 0.0, 0.0)
    off = np.float32((32.0 - 20.0) / 32.0) - np.float32(h)
    out = om.composite(frame(), u, tex, 5, om.Layers().points([[0.0, off, 0.0]], size_px=2, rgba=(0, 0, 0, 255), drape=True))
    ys, _ = changed(out).T
    assert set(ys.tolist()) <= {18, 19, 20, 21} and 19 in ys and 20 in ys
