"""The geometry-buffer CPU model (tests/gbuffer_model) against the contract of DESIGN.md 4f, on visibility drawn by the oracle: the
model is what the GPU planes are held to bit for bit (tests/test_gpu_gbuffer.py).  No GPU needed.

Reprojection bounds.  `position` is interpolated inside the SNAPPED triangle (vertices moved by up to 1/512 px per axis, DESIGN.md 4
item 4) but lies on the unsnapped one in the world, so projecting it back misses the pixel centre by about the snap, amplified by
the triangle's depth range.  The bounds below are twice the largest errors of the model over the six fixed scenes of this file
(measured: 0.002666 px, relative w error 3.83e-7; DESIGN.md 4f has the table); the factor two is room for a later scene.
"""

import numpy as np
import pytest

import support  # noqa: F401  (the repository root and the model directories on sys.path)
import gbuffer_model as gbm
import oracle

ocm, om = gbm.ocm, gbm.om
GRID = 256
LUT = np.zeros(1024, np.uint8)
CAMERAS = {
    "default": ((3.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0),
    "fill": ((0.0, 2.2, 0.01), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 0.1, 100.0),
    "near": ((0.2, 0.6, 0.1), (1.5, 0.2, 1.2), (0.0, 1.0, 0.0), 70.0, 0.5, 100.0),
}
SIZES = [(320, 200), (257, 131)]
PX_BOUND = 2 * 0.002666                                       # pixels
W_BOUND = 2 * 3.83e-7                                         # relative


def bumpy(seed=7, shape=(67, 71)):
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) * 0.6 - 0.3).astype(np.float32)


_frames = {}


def frame(cam, size, flat=False):
    """(uniforms, height, visibility, depth, position, normal) of one scene, cached"""
    key = (cam, size, flat)
    if key not in _frames:
        W, H = size
        u = oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam])
        h = np.zeros((8, 8), np.float32) if flat else bumpy()
        if flat:
            u = u.copy()
            u[38] = 0.0                                       # no exaggeration: the analytic part of the displaced height is flat too
        vis = oracle.render_terrain(u, W, H, GRID, h, LUT, want_vis=True, nthreads=8)[1]
        _frames[key] = (u, h, vis) + gbm.planes(vis, u, h, GRID)
    return _frames[key]


def reproject(u, position, W, H):
    """float64: pixel coordinates and clip w of the world positions under proj * view of the uniform block"""
    M = u[16:32].reshape(4, 4).T.astype(np.float64) @ u[0:16].reshape(4, 4).T.astype(np.float64)
    c = np.concatenate([position.astype(np.float64), np.ones(position.shape[:-1] + (1,))], axis=-1) @ M.T
    return (c[..., 0] / c[..., 3] + 1) * W / 2, (1 - c[..., 1] / c[..., 3]) * H / 2, c[..., 3]


SCENES = [(c, s) for c in CAMERAS for s in SIZES]


@pytest.mark.parametrize("cam,size", SCENES)
def test_depth_is_the_reciprocal_of_the_occlusion_models_q(cam, size):
    u, h, vis, depth, _, _ = frame(cam, size)
    Q, clipped = ocm.terrain_q(vis, u, h, GRID)
    cov = vis != 0
    assert cov.any() and (~cov).any()
    assert np.array_equal(depth[cov].view(np.uint32), (np.float32(1.0) / Q[cov]).view(np.uint32))
    assert np.array_equal(np.isposinf(depth), ~cov)
    assert (depth[cov] > 0).all()
    if cam == "near":
        assert (clipped & cov).any()                          # the generic path is exercised


@pytest.mark.parametrize("cam,size", SCENES)
def test_position_reprojects_onto_the_pixel_centre_at_its_depth(cam, size):
    W, H = size
    u, h, vis, depth, position, _ = frame(cam, size)
    cov = vis != 0
    sx, sy, w = reproject(u, position, W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    err = np.hypot(sx - (xx + 0.5), sy - (yy + 0.5))[cov]     # every covered pixel, clipped primitives included
    werr = (np.abs(w - depth.astype(np.float64))[cov] / depth[cov])
    print(f"{cam} {W}x{H}: {int(cov.sum())} covered, max pixel error {err.max():.6f}, max relative w error {werr.max():.3e}")
    assert err.max() <= PX_BOUND
    assert werr.max() <= W_BOUND
    assert not position[~cov].any()


def float64_normals(u, h, ids):
    """unit normals (float64, pointing up) of the primitives `ids` (visibility ids), rebuilt from the vertex heights and grid coordinates"""
    nm1 = GRID - 1
    step = np.float32(3.0) / np.float32(nm1)
    tex = np.ascontiguousarray(h, np.float32)
    hgt = lambda i, j: float(om.lib().ovm_vertex_height(tex, tex.shape[1], tex.shape[0], GRID, int(i), int(j)))
    xz = lambda i: float(np.float32(-1.5) + np.float32(i) * step) * float(max(u[36], np.float32(1e-8)))
    out = np.zeros((len(ids), 3))
    for k, vid in enumerate(ids):
        prim = int(vid) - 1
        cell, odd = prim >> 1, prim & 1
        j, i = divmod(cell, nm1)
        vs = [(i + odd, j), (i, j + 1), (i + 1, j + odd)]
        P = np.array([[xz(a), hgt(a, b) * float(u[38]), xz(b)] for a, b in vs])
        n = np.cross(P[1] - P[0], P[2] - P[0])
        n = -n if n[1] < 0 else n
        out[k] = n / np.linalg.norm(n)
    return out


@pytest.mark.parametrize("cam,size", SCENES)
def test_normal_is_the_unit_geometric_normal_of_the_visible_triangle(cam, size):
    u, h, vis, _, _, normal = frame(cam, size)
    cov = vis != 0
    n = normal[cov].astype(np.float64)
    assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 4 * 2.0 ** -24).all()
    assert (normal[cov][:, 1] >= 0).all()
    assert not normal[~cov].any()
    ids, first, inverse = np.unique(vis[cov], return_index=True, return_inverse=True)
    per_id = normal[cov][first]
    assert np.array_equal(per_id[inverse].view(np.uint32), normal[cov].view(np.uint32))       # constant over a primitive's pixels
    assert np.abs(per_id - float64_normals(u, h, ids)).max() <= 1e-5


def test_a_flat_field_seen_from_above():
    """Zero heights and zero exaggeration under the `fill` camera: the surface is the plane y = 0.  The camera looks down from 2.2
    above the plane, tilted by atan(0.01 / 2.2), and `depth` is clip w under the frame's own projection, so it is not 2.2 everywhere: it
    is held, within the reprojection bound, to the float64 clip w of the plane along each pixel's own ray, and at the frame's centre to
    the clip w of the camera's target."""
    W, H = SIZES[0]
    u, h, vis, depth, position, normal = frame("fill", SIZES[0], flat=True)
    cov = vis != 0
    assert cov.mean() > 0.3
    assert (position[cov][:, 1] == 0).all()
    assert (normal[cov] == np.float32([0, 1, 0])).all()
    V = u[0:16].reshape(4, 4).T.astype(np.float64)
    Pm = u[16:32].reshape(4, 4).T.astype(np.float64)
    inv = np.linalg.inv(Pm @ V)
    yy, xx = np.mgrid[0:H, 0:W]
    ndc = np.stack([(xx + 0.5) / W * 2 - 1, 1 - (yy + 0.5) / H * 2], axis=-1)
    a = np.concatenate([ndc, np.full((H, W, 1), 0.25), np.ones((H, W, 1))], axis=-1) @ inv.T
    b = np.concatenate([ndc, np.full((H, W, 1), 0.75), np.ones((H, W, 1))], axis=-1) @ inv.T
    a, b = a[..., :3] / a[..., 3:], b[..., :3] / b[..., 3:]
    t = a[..., 1] / (a[..., 1] - b[..., 1])                   # the ray meets y = 0
    hit = a + t[..., None] * (b - a)
    w = (np.concatenate([hit, np.ones((H, W, 1))], axis=-1) @ (Pm @ V).T)[..., 3]
    rel = np.abs(w - depth.astype(np.float64))[cov] / w[cov]
    print(f"flat: max relative depth error against the plane {rel.max():.3e}")
    assert rel.max() <= W_BOUND
    # the camera's target, the origin, lies on the plane and on the view axis: the four pixels round the principal point are half a pixel
    # off it on a plane tilted by 0.26 degrees, 1.4e-5 of the depth
    w0 = ((Pm @ V) @ np.array([0.0, 0.0, 0.0, 1.0]))[3]
    centre = depth[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].astype(np.float64)
    assert np.abs(centre - w0).max() <= w0 * (W_BOUND + 2e-5)


def test_pick_equals_the_planes():
    W, H = SIZES[1]
    u, h, vis, depth, position, normal = frame("near", SIZES[1])
    rng = np.random.default_rng(5)
    px = np.column_stack([rng.integers(0, W, 500), rng.integers(0, H, 500)])
    px = np.concatenate([px, [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]])
    got = gbm.pick(px, vis, u, h, GRID)
    at = (px[:, 1], px[:, 0])
    for name, plane in (("depth", depth), ("position", position), ("normal", normal), ("primitive", vis)):
        assert np.array_equal(got[name].view(np.uint32), plane[at].view(np.uint32)), name
    with pytest.raises(ValueError):
        gbm.pick([[W, 0]], vis, u, h, GRID)
