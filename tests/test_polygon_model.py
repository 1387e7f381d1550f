"""The polygon fill CPU model (tests/polygon_model) against the contract of DESIGN.md 4c, and the argument rules of pack_polygons /
add_polygons: the model is what the GPU frames are held to bit for bit (tests/test_gpu_polygons.py), so its behaviour is pinned here
against an independent float64 evaluation and hand-worked cases.  No GPU needed."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
import support  # noqa: F401  (the repository root and the model directories on sys.path)
import polygon_model as pm
om = pm.om

_spec = importlib.util.spec_from_file_location("vf_overlay_rules", os.path.join(os.path.dirname(HERE), "vulkan_forge_amd", "_overlays.py"))
ov = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ov)

TEX = np.zeros((1, 1), np.float32)
BG = np.array([90, 60, 30, 255], np.uint8)


def ortho(W, H, z_from_x=False):
    """view = identity, clip = (x, y, 0.5, 1) -- or (x, y, x, 1): the near plane z >= 0 is then x >= 0.  Screen = (W/2 (1 + x), H/2 (1 - y))."""
    u = np.zeros(44, np.float32)
    u[0:16] = np.eye(4, dtype=np.float32).reshape(16)
    proj = np.zeros(16, np.float32)                         # column-major
    proj[0], proj[5], proj[15] = 1.0, 1.0, 1.0
    if z_from_x:
        proj[2] = 1.0
    else:
        proj[14] = 0.5
    u[16:32] = proj
    u[36], u[38] = 1.0, 1.0
    return u


def world(W, H, pts):
    """screen points (k, 2) -> world (k, 3) under ortho(W, H)"""
    pts = np.asarray(pts, np.float64)
    return np.column_stack([pts[:, 0] / (W / 2) - 1.0, 1.0 - pts[:, 1] / (H / 2), np.zeros(len(pts))]).astype(np.float32)


def screen(W, H, xyz):
    """world (k, 3) float32 -> screen (k, 2) float64, the exact map of ortho(W, H)"""
    xyz = np.asarray(xyz, np.float64)
    return np.column_stack([(xyz[:, 0] + 1.0) * (W / 2), (1.0 - xyz[:, 1]) * (H / 2)])


def ngon(cx, cy, r, n, phase=0.1, reverse=False):
    a = phase + 2 * np.pi * np.arange(n) / n
    p = np.column_stack([cx + r * np.cos(a), cy + r * np.sin(a)])
    return p[::-1] if reverse else p


def numpy_coverage(W, H, rings_screen):
    """independent float64 evaluation of 4c: even-odd parity of crossings right of each pixel centre, nearest-edge distance"""
    qx, qy = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    par = np.zeros((H, W), bool)
    d2 = np.full((H, W), np.inf)
    for ring in rings_screen:
        a, b = ring, np.roll(ring, -1, axis=0)
        for (x0, y0), (x1, y1) in zip(a, b):
            ex, ey = x1 - x0, y1 - y0
            if (y0 <= qy[:, :1]).any() or True:
                crosses = (y0 <= qy) != (y1 <= qy)
                with np.errstate(divide="ignore", invalid="ignore"):
                    xc = x0 + (qy - y0) * ex / ey
                par ^= crosses & (xc > qx)
            t = np.clip(((qx - x0) * ex + (qy - y0) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
            d2 = np.minimum(d2, (qx - x0 - t * ex) ** 2 + (qy - y0 - t * ey) ** 2)
    d = np.sqrt(d2)
    return np.clip(0.5 - np.where(par, -d, d), 0.0, 1.0)


def shoelace(p):
    x, y = p[:, 0], p[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def model_coverage(W, H, rings_screen, u=None):
    return pm.fill_coverage(W, H, ortho(W, H) if u is None else u, TEX, 2, [world(W, H, r) for r in rings_screen])


# ---- pack_polygons and the argument rules --------------------------------------------------------

def test_pack_polygons_donut_multipolygon_and_cleanup():
    sq = np.array([[0, 0, 0], [4, 0, 0], [4, 0, 4], [0, 0, 4]], np.float64)
    hole = np.array([[1, 0, 1], [1, 0, 1], [2, 0, 1], [2, 0, 2], [1, 0, 2], [1, 0, 1]], np.float32)   # duplicate + closing vertex
    other = sq + [10, 0, 0]
    coords, rings, feats = ov.pack_polygons([[sq, hole], [sq + [20, 0, 0], other], np.vstack([sq, sq[:1]])])
    assert coords.dtype == np.float32 and rings.dtype == np.uint32 and feats.dtype == np.uint32
    assert rings.tolist() == [0, 4, 8, 12, 16, 20]
    assert feats.tolist() == [0, 2, 4, 5]                    # donut (exterior + hole), a two-part multipolygon, a closed ring
    assert coords[4:8].tolist() == [[1, 0, 1], [2, 0, 1], [2, 0, 2], [1, 0, 2]]
    assert coords[16:20].tolist() == sq.tolist()             # (the closing vertex is gone)
    c1, r1, f1 = ov.pack_polygons(np.stack([sq, other]))     # an (F, k, 3) array: F single-ring polygons
    assert r1.tolist() == [0, 4, 8] and f1.tolist() == [0, 1, 2]
    c2, r2, f2 = ov.pack_polygons(sq)                        # one (k, 3) array: one polygon
    assert r2.tolist() == [0, 4] and f2.tolist() == [0, 1]
    c3, r3, f3 = ov.pack_polygons([])
    assert c3.shape == (0, 3) and r3.tolist() == [0] and f3.tolist() == [0]


def test_pack_polygons_refusals():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    with pytest.raises(ValueError, match=r"polygon 1 ring 0 has fewer than 3 distinct vertices"):
        ov.pack_polygons([tri, np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]], np.float32)])
    with pytest.raises(ValueError, match=r"polygon 0 ring 1 has fewer than 3 distinct vertices"):
        ov.pack_polygons([[tri, np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)]])
    with pytest.raises(ValueError, match=r"polygon 0 ring 0 has a non-finite coordinate"):
        ov.pack_polygons([np.array([[0, 0, 0], [1, 0, 0], [0, np.nan, 1]], np.float32)])
    with pytest.raises(ValueError, match=r"polygon 0 ring 0 has a non-finite coordinate"):
        ov.pack_polygons([np.array([[0, 0, 0], [np.inf, 0, 0], [0, 0, 1]], np.float32)])
    with pytest.raises(ValueError, match=r"polygon 0 has no ring"):
        ov.pack_polygons([[]])
    with pytest.raises(TypeError, match="float32 or float64"):
        ov.pack_polygons([tri.astype(np.int32)])
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
        ov.pack_polygons([np.zeros((4, 2), np.float32)])


def test_polygon_args():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    with pytest.raises(ValueError, match="cannot both be None"):
        ov.polygon_args([tri], None, None, 1.0)
    with pytest.raises(ValueError, match=r"\(2, 4\)"):
        ov.polygon_args([tri, tri], np.zeros((3, 4), np.uint8), None, 1.0)
    with pytest.raises(TypeError, match="uint8"):
        ov.polygon_args([tri], np.zeros((1, 4), np.float32), None, 1.0)
    with pytest.raises(ValueError, match="0..255"):
        ov.polygon_args([tri], (0, 0, 0, 300), None, 1.0)
    with pytest.raises(ValueError, match="4-tuple"):
        ov.polygon_args([tri], (1, 2, 3, 4), np.zeros((1, 4), np.uint8), 1.0)
    with pytest.raises(ValueError, match="positive finite"):
        ov.polygon_args([tri], (1, 2, 3, 4), (1, 2, 3, 4), -1.0)
    with pytest.raises(TypeError, match="line_width_px must be a number"):
        ov.polygon_args([tri], (1, 2, 3, 4), None, "2")
    coords, rings, feats, dfill, fills, line, width = ov.polygon_args([tri, tri], (1, 2, 3, 4), None, 2.0)
    assert dfill.tolist() == [1, 2, 3, 4] and fills is None and line is None and width == 2.0
    coords, rings, feats, dfill, fills, line, width = ov.polygon_args([tri, tri], np.full((2, 4), 7, np.uint8), (9, 9, 9, 9), 1.0)
    assert dfill is None and fills.shape == (2, 4) and line.tolist() == [9, 9, 9, 9]


# ---- the model against the contract --------------------------------------------------------------

@pytest.mark.parametrize("case", ["triangle", "donut", "multipolygon", "star"])
def test_model_coverage_matches_a_float64_brute_force(case):
    W, H = 64, 48
    rings = {
        "triangle": [np.array([[5.3, 4.1], [58.7, 11.6], [21.2, 44.9]])],
        "donut": [ngon(31.7, 23.9, 20.3, 40), ngon(30.2, 24.6, 8.4, 23, 0.7, reverse=True)],
        "multipolygon": [ngon(15.2, 15.1, 11.3, 7), ngon(46.6, 30.3, 13.8, 11, 0.4), np.array([[-9.5, 40.2], [80.1, 42.7], [30.3, 70.4]])],
        "star": [ngon(32.1, 24.2, 21.7, 5, 0.3)[[0, 2, 4, 1, 3]]],
    }[case]
    got = model_coverage(W, H, rings)
    want = numpy_coverage(W, H, [screen(W, H, world(W, H, r)) for r in rings])
    assert 0.0 < got.sum() and np.abs(got - want).max() <= 1e-4


@pytest.mark.parametrize("case", ["triangle", "donut"])
def test_coverage_sums_to_the_screen_area(case):
    W, H = 256, 192
    if case == "triangle":
        rings = [np.array([[17.3, 12.9], [231.4, 40.2], [90.8, 170.5]])]
        area = shoelace(rings[0])
    else:
        rings = [ngon(128.3, 95.7, 80.2, 256), ngon(120.1, 99.4, 35.6, 128, 0.2)]
        area = shoelace(rings[0]) - shoelace(rings[1])
    got = model_coverage(W, H, rings).astype(np.float64).sum()
    assert abs(got - area) <= 0.005 * area, (got, area)


def test_even_odd_bow_tie_and_pentagram():
    W, H = 64, 64
    bow = [np.array([[8.2, 8.3], [56.1, 55.7], [56.3, 8.1], [8.1, 56.2]])]          # self-intersecting: two lobes
    cov = model_coverage(W, H, bow)
    assert cov[32, 12] == 1.0 and cov[32, 52] == 1.0                             # left and right lobes inside
    assert cov[12, 32] == 0.0 and cov[52, 32] == 0.0                             # top and bottom wedges outside
    star = [ngon(32.0, 32.0, 28.0, 5, 0.31)[[0, 2, 4, 1, 3]]]
    cov = model_coverage(W, H, star)
    assert cov[32, 32] == 0.0                                                    # even-odd: the centre pentagon is a hole
    tip = ngon(32.0, 32.0, 22.0, 5, 0.31)[0]
    assert cov[int(tip[1]), int(tip[0])] == 1.0                                  # the points are inside
    overlap = [ngon(24.2, 32.1, 14.3, 32), ngon(40.3, 32.2, 14.1, 32)]           # two rings overlapping in one feature
    cov = model_coverage(W, H, overlap)
    assert cov[32, 32] == 0.0 and cov[32, 14] == 1.0 and cov[32, 50] == 1.0


def test_near_plane_clip_matches_a_hand_worked_edge_set():
    # clip z = world x: the near plane z >= 0 keeps x >= 0.  Square (-0.5, -0.5) .. (0.5, 0.5) on a 64 x 64 frame, screen = 32 + 32 x,
    # 32 - 32 y.  Edge 0 (-.5,-.5) -> (.5,-.5) enters at (0, -.5); edge 1 is kept whole; edge 2 (.5,.5) -> (-.5,.5) exits at (0, .5);
    # edge 3 is behind; the exit closes along the plane to the next entry, (0, -.5).
    u = ortho(64, 64, z_from_x=True)
    ring = np.array([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.0]], np.float32)
    E = pm.ring_edges(64, 64, u, TEX, 2, ring)
    ends = [(e[0], e[1], e[0] + e[2], e[1] + e[3]) for e in E]
    assert ends == [(32.0, 48.0, 48.0, 48.0), (48.0, 48.0, 48.0, 16.0), (48.0, 16.0, 32.0, 16.0), (32.0, 16.0, 32.0, 48.0)]
    assert E[1][5] == 0.0 and E[0][5] == 0.0 and E[1][4] == np.float32(1.0 / 1024.0)     # ex / ey, 1 / |e|^2
    assert len(pm.ring_edges(64, 64, u, TEX, 2, ring - [1.0, 0.0, 0.0])) == 0       # wholly behind the plane: nothing
    # a ring crossing the plane twice in each direction (a "W"): two closing segments
    w = np.array([[-0.5, -0.6, 0], [0.6, -0.6, 0], [0.6, -0.2, 0], [-0.4, -0.1, 0], [0.6, 0.2, 0], [0.6, 0.6, 0], [-0.5, 0.6, 0]], np.float32)
    E = pm.ring_edges(64, 64, u, TEX, 2, w)
    vertical = [e for e in E if e[2] == 0.0 and e[0] == 32.0]
    assert len(vertical) == 2                                                    # both closing segments lie on x = 0 (screen 32)
    cov = pm.fill_coverage(64, 64, u, TEX, 2, [w])
    assert cov[:, :31].max() == 0.0 and cov[32, 40] == 0.0 and cov[20, 40] == 1.0 and cov[45, 40] == 1.0


def test_outline_only_equals_the_line_model_of_the_closed_rings():
    W, H = 96, 64
    u = ortho(W, H)
    polys = [[world(W, H, ngon(30.2, 30.1, 20.4, 9)), world(W, H, ngon(31.2, 29.8, 7.7, 5, 0.5))], world(W, H, ngon(70.3, 35.2, 18.1, 4))]
    frame = np.broadcast_to(BG, (H, W, 4)).copy()
    got = pm.composite(frame, u, TEX, 2, pm.Layers().polygons(polys, fill_rgba=None, line_rgba=(250, 240, 10, 200), line_width_px=3.0))
    closed = [np.vstack([r, r[:1]]) for r in [polys[0][0], polys[0][1], polys[1]]]
    want = om.composite(frame, u, TEX, 2, om.Layers().lines(closed, width_px=3.0, rgba=(250, 240, 10, 200), cap="round"))
    assert not np.array_equal(got, frame) and np.array_equal(got, want)


def test_fill_layers_keep_feature_order_with_points_and_lines():
    W, H = 64, 64
    u = ortho(W, H)
    frame = np.broadcast_to(BG, (H, W, 4)).copy()
    sq = world(W, H, np.array([[10.2, 10.3], [50.1, 10.2], [50.3, 50.2], [10.1, 50.4]]))
    pts = world(W, H, np.array([[30.0, 30.0]]))
    under = pm.composite(frame, u, TEX, 2, pm.Layers().points(pts, size_px=10, rgba=(255, 0, 0, 255)).polygons([sq], fill_rgba=(0, 0, 255, 255)))
    over = pm.composite(frame, u, TEX, 2, pm.Layers().polygons([sq], fill_rgba=(0, 0, 255, 255)).points(pts, size_px=10, rgba=(255, 0, 0, 255)))
    assert under[30, 30].tolist() == [0, 0, 255, 255] and over[30, 30].tolist() == [255, 0, 0, 255]
    # without fills the model is the overlay model
    L = pm.Layers().points(pts, size_px=7, rgba=(1, 200, 3, 150)).lines([world(W, H, ngon(30, 30, 20, 6))], width_px=2.5)
    assert np.array_equal(pm.composite(frame, u, TEX, 2, L), om.composite(frame, u, TEX, 2, L))


def test_translucent_fill_blends_once_per_pixel():
    W, H = 48, 48
    u = ortho(W, H)
    frame = np.broadcast_to(BG, (H, W, 4)).copy()
    # two overlapping rings of one feature: the overlap is outside (even-odd); each pixel is blended once with its fill coverage
    poly = [world(W, H, ngon(20.1, 24.2, 12.3, 24)), world(W, H, ngon(28.2, 24.1, 12.2, 24))]
    out = pm.composite(frame, u, TEX, 2, pm.Layers().polygons([poly], fill_rgba=(255, 255, 255, 128)))
    cov = model_coverage(W, H, [screen(W, H, r) for r in poly])  # (the same polygon; screen() -> world() round trip is exact here)
    a = np.float32(128) / np.float32(255)
    for y, x in [(24, 12), (24, 36), (24, 24), (5, 5)]:
        c = np.float32(cov[y, x]) * a
        want = [om.encode(np.float32(om.decode(255)) * c + np.float32(om.decode(int(BG[k]))) * (np.float32(1) - c)) if cov[y, x] > 0 else int(BG[k])
                for k in range(3)]
        assert out[y, x, :3].tolist() == want, (y, x)
