"""The occlusion CPU model (tests/occlusion_model) against the contract of DESIGN.md 4d, on frames and visibility drawn by the oracle:
the model is what the GPU frames are held to bit for bit (tests/test_gpu_occlusion.py).  No GPU needed."""

import numpy as np
import pytest

from support import ridge
import occlusion_model as ocm
import oracle

pm, om = ocm.pm, ocm.om
GRID = 256
LUT = np.column_stack([np.arange(256)] * 3 + [np.full(256, 255)]).astype(np.uint8).reshape(1024)
CAMERAS = {
    "default": ((3.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0),
    "fill": ((0.0, 2.2, 0.01), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 0.1, 100.0),
    "near": ((0.2, 0.6, 0.1), (1.5, 0.2, 1.2), (0.0, 1.0, 0.0), 70.0, 0.5, 100.0),
    "ridge": ((0.0, 1.0, 3.0), (0.0, 0.3, 0.0), (0.0, 1.0, 0.0), 50.0, 0.1, 100.0),
}


def bumpy(seed=7, shape=(67, 71)):
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) * 0.6 - 0.3).astype(np.float32)


def terrain(cam, h, W=240, H=160):
    u = oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam])
    rgba, vis = oracle.render_terrain(u, W, H, GRID, h, LUT, want_vis=True, nthreads=8)
    return u, rgba, vis


def draped_points(rng, n, lo=-1.4, hi=1.4, y=0.0):
    return np.column_stack([rng.uniform(lo, hi, n), np.full(n, y), rng.uniform(lo, hi, n)]).astype(np.float32)


def centre_pixels(u, h, xyz, W, H):
    """(n, 2) pixel (x, y) holding each draped point's projected centre (float64: a locator, not the contract)"""
    M = u[16:32].reshape(4, 4).T.astype(np.float64) @ u[0:16].reshape(4, 4).T.astype(np.float64)
    y = [om.drape(u, h, GRID, p[0], p[2]) + p[1] for p in xyz]
    c = np.column_stack([xyz[:, 0], y, xyz[:, 2], np.ones(len(xyz))]) @ M.T
    px = np.column_stack([(c[:, 0] / c[:, 3] + 1) * W / 2, (1 - c[:, 1] / c[:, 3]) * H / 2])
    return np.floor(px).astype(int)


def mixed(occlude_every=None, bias=ocm.DEPTH_BIAS, seed=3):
    """points, lines and polygons; the point / line layers occlude where occlude_every picks them"""
    rng = np.random.default_rng(seed)
    L = ocm.Layers()
    k = 0
    for drape in (True, False):
        for shape in ("circle", "square"):
            xyz = draped_points(rng, 300, y=0.02 if drape else 0.4)
            L.points(xyz, size_px=float(3 + 2 * k), rgba=(40 * k, 200, 90, 255 - 30 * k), shape=shape, drape=drape,
                     occlude=occlude_every is not None and k % occlude_every == 0, depth_bias=bias)
            k += 1
        paths = [(np.array([rng.uniform(-1.4, 1.4), 0.03, rng.uniform(-1.4, 1.4)]) + np.cumsum(rng.normal(0, 0.1, (6, 3)) * [1, 0, 1], axis=0)).astype(np.float32)
                 for _ in range(40)]
        L.lines(paths, width_px=3.0, rgba=(250, 60 * k % 255, 20, 200), cap=("round", "square")[k % 2], drape=drape,
                occlude=occlude_every is not None and k % occlude_every == 0, depth_bias=bias)
        k += 1
        L.polygons([np.array([[-0.5, 0.05, -0.5], [0.6, 0.05, -0.4], [0.1, 0.05, 0.7]], np.float32)], fill_rgba=(0, 90, 255, 120),
                   line_rgba=(0, 0, 0, 255), line_width_px=2.0, drape=drape)
    return L


@pytest.mark.parametrize("cam", ["default", "fill", "near"])
def test_non_occluding_layers_equal_the_overlay_and_polygon_models(cam):
    h = bumpy()
    u, base, vis = terrain(cam, h)
    L = mixed()
    got = ocm.composite(base, vis, u, h, GRID, L)
    assert np.array_equal(got, pm.composite(base, u, h, GRID, L))
    assert not np.array_equal(got, base)
    P = ocm.Layers()
    P.points(draped_points(np.random.default_rng(1), 500, y=0.1), size_px=5, rgba=(255, 0, 0, 200), drape=True)
    P.lines([np.array([[-1.4, 0.2, -1.4], [1.4, 0.3, 1.4], [1.4, 0.1, -1.4]], np.float32)], width_px=4, cap="square")
    assert np.array_equal(ocm.composite(base, vis, u, h, GRID, P), om.composite(base, u, h, GRID, P))


def test_a_ridge_hides_what_lies_behind_it_and_nothing_in_front():
    h = ridge()
    u, base, vis = terrain("ridge", h)
    xs = np.linspace(-1.2, 1.2, 25, dtype=np.float32)
    behind = np.column_stack([xs, np.full(25, 0.02, np.float32), np.full(25, -0.9, np.float32)])
    front = behind * np.float32([1, 1, -1])
    for occl_layer in (lambda L: L.points(behind, size_px=6, rgba=(255, 0, 0, 255), drape=True, occlude=True),
                       lambda L: L.lines([behind], width_px=5, rgba=(255, 0, 0, 255), drape=True, occlude=True)):
        L = ocm.Layers()
        occl_layer(L)
        assert np.array_equal(ocm.composite(base, vis, u, h, GRID, L), base)        # behind the ridge: not a pixel changes
        L.set_occlusion(0, False)
        assert (ocm.composite(base, vis, u, h, GRID, L) != base).any(axis=2).sum() > 200   # (drawn over the ridge without occlusion)
    for layer in (lambda L: L.points(front, size_px=6, rgba=(255, 0, 0, 255), drape=True, occlude=True),
                  lambda L: L.lines([front], width_px=5, rgba=(255, 0, 0, 255), drape=True, occlude=True)):
        L = ocm.Layers()
        layer(L)
        drawn = (ocm.composite(base, vis, u, h, GRID, L) != base).any(axis=2)
        assert drawn.sum() > 200
        assert drawn[tuple(centre_pixels(u, h, front, *base.shape[1::-1]).T[::-1])].all()   # in front of it: every vertex drawn


def test_background_never_hides():
    h = bumpy()
    u, base, vis = terrain("default", h)
    Q, _ = ocm.terrain_q(vis, u, h, GRID)
    assert (Q[vis == 0] == 0).all() and (Q[vis != 0] > 0).all()
    # points far behind the terrain, in the sky of the frame: nothing is in front of them
    rng = np.random.default_rng(4)
    sky = np.column_stack([rng.uniform(-30, 0, 400), rng.uniform(4, 12, 400), rng.uniform(-30, 0, 400)]).astype(np.float32)
    L = ocm.Layers().points(sky, size_px=5, rgba=(255, 255, 0, 255), occlude=True, depth_bias=0.0)
    got = ocm.composite(base, vis, u, h, GRID, L)
    drawn = (got != base).any(axis=2)
    assert drawn.sum() > 1000 and (vis[drawn] == 0).all()
    L.set_occlusion(0, False)
    assert np.array_equal(got, ocm.composite(base, vis, u, h, GRID, L))


def test_hidden_pixels_only_grow_as_depth_bias_falls():
    h = bumpy(9)
    u, base, vis = terrain("default", h)
    rng = np.random.default_rng(6)
    pts = draped_points(rng, 3000, y=0.0)
    paths = [(np.array([rng.uniform(-1.4, 1.4), 0.0, rng.uniform(-1.4, 1.4)]) + np.cumsum(rng.normal(0, 0.15, (5, 3)) * [1, 0, 1], axis=0)).astype(np.float32)
             for _ in range(60)]
    plain = ocm.composite(base, vis, u, h, GRID, ocm.Layers().points(pts, size_px=3, drape=True).lines(paths, width_px=2, drape=True))
    prev, counts = None, []
    for bias in (1.0, 0.1, 0.01, 1e-3, 1e-4, 0.0):
        L = ocm.Layers().points(pts, size_px=3, drape=True, occlude=True, depth_bias=bias).lines(paths, width_px=2, drape=True, occlude=True,
                                                                                               depth_bias=bias)
        hidden = (ocm.composite(base, vis, u, h, GRID, L) != plain).any(axis=2)
        if prev is not None:
            assert not (prev & ~hidden).any(), f"depth_bias {bias}: a pixel hidden at a larger bias is drawn"
        prev = hidden
        counts.append(int(hidden.sum()))
    assert counts[0] < counts[-1]


def test_near_camera_hides_behind_near_clipped_terrain():
    h = bumpy()
    u, base, vis = terrain("near", h)
    Q, clipped = ocm.terrain_q(vis, u, h, GRID)
    assert clipped.any()
    rng = np.random.default_rng(8)
    pts = np.column_stack([rng.uniform(0.1, 1.5, 8000), np.full(8000, -0.05), rng.uniform(0.1, 1.5, 8000)]).astype(np.float32)
    L = ocm.Layers().points(pts, size_px=4, rgba=(255, 0, 255, 255), drape=True, occlude=True)
    got = ocm.composite(base, vis, u, h, GRID, L)
    L.set_occlusion(0, False)
    plain = ocm.composite(base, vis, u, h, GRID, L)
    hidden = (got != plain).any(axis=2)
    assert (hidden & clipped).sum() > 20                     # the generic (clipped) path decided these


def test_default_depth_bias_keeps_draped_points_on_a_front_slope_visible():
    """Draped points (offset 0) on the ridge's front slope: the pixel that holds each centre is drawn at the default depth_bias (at
    1e-3, 44 of these 125 are not: a disc is flat at its centre's depth while the slope under it recedes)."""
    h = ridge()
    u, base, vis = terrain("ridge", h, 320, 200)
    g = np.linspace(-1.2, 1.2, 25)
    pts = np.array([[x, 0.0, z] for x in g for z in (0.5, 0.7, 0.9, 1.1, 1.3)], np.float32)
    at = tuple(centre_pixels(u, h, pts, 320, 200).T[::-1])
    for size in (1, 6):
        for bias, all_drawn in ((ocm.DEPTH_BIAS, True), (1e-3, False)):
            L = ocm.Layers().points(pts, size_px=size, rgba=(255, 0, 0, 255), drape=True, occlude=True, depth_bias=bias)
            drawn = (ocm.composite(base, vis, u, h, GRID, L) != base).any(axis=2)
            assert drawn[at].all() == all_drawn, (size, bias)
