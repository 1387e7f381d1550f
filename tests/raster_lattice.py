"""Whole terrain frames whose grid vertices land exactly on pixel centres: the uniform blocks, the lattice each one is meant to
produce and an integer evaluation of the coverage rule on that lattice.  Shared by tests/test_raster_lattice.py (CPU: the cases
are what they claim to be) and tests/test_gpu_raster_device.py (GPU: the HIP frame equals the oracle's).

The camera is an affine map with w = 1: view = identity, spacing 1, exaggeration 0 (every height becomes 0), and a projection whose
rows 0 / 1 carry a 2 x 2 matrix and a translation, row 2 the constant depth 0.5, row 3 (0, 0, 0, 1).  Grid vertex (i, j) is meant to
land on pixel position  P = M (i, j) + t  with M = cell * (a rotation by a multiple of 90 degrees, or the shear that makes the
cells' diagonals vertical) and t on the half-pixel lattice, so that P is a pixel centre (cell 8 and 1) or a pixel centre / the
middle of a pixel edge (cell 0.5).  The matrix entries are not all exact in binary32 (1 / 48 and 1 / 40 are not), but the error
of the float vertex stage stays four orders of magnitude below the 1 / 512 pixel the 24.8 snap forgives: the CPU test restates
that stage in float32 and requires the snapped vertices to BE the lattice."""
import numpy as np

W, H = 96, 80                       # one and a half tiles by one and a quarter: lattice lines cross a tile boundary in both axes
GRID = {8.0: 13, 1.0: 97, 0.5: 193}  # cells per side 12, 96, 192 = 3 * 2^k: the grid pitch 3 / (n - 1) is a power of two
ORIENT = {"rot0": ((1, 0), (0, 1)), "rot90": ((0, -1), (1, 0)), "rot180": ((-1, 0), (0, -1)), "rot270": ((0, 1), (-1, 0)),
          "shear": ((1, 1), (0, 1))}  # all of determinant +1: the triangles stay front-facing; shear: the diagonal (1, -1) maps to (0, -1)
CASES = [(cell, name) for cell in (8.0, 1.0, 0.5) for name in ORIENT]


def lattice(cell, name):
    """(n, M, t): P(i, j) = M @ (i, j) + t in pixels.  The lattice's bounding box starts 10.5 pixels left of the target and 6.5 pixels
    below its top (12.5 left for the shear, whose box is twice as wide): part of it is off-screen, part of the screen stays background."""
    n = GRID[cell]
    M = cell * np.array(ORIENT[name], np.float64)
    corners = np.array([[0, 0], [n - 1, 0], [0, n - 1], [n - 1, n - 1]], np.float64) @ M.T
    t = np.array([-60.5 if name == "shear" else -10.5, 6.5]) - corners.min(axis=0)
    return n, M, t


def uniforms(cell, name):
    """The 44-float uniform block (view, proj, sun, exposure, spacing, h_range, exaggeration, pad) of the case."""
    n, M, t = lattice(cell, name)
    step = 3.0 / (n - 1)
    hw, hh = 0.5 * W, 0.5 * H
    t0 = t + 1.5 * M.sum(axis=1) / step                    # i = (x + 1.5) / step
    proj = np.zeros(16, np.float64)                        # column-major: m[4 * column + row]
    proj[0], proj[8], proj[12] = M[0, 0] / (step * hw), M[0, 1] / (step * hw), t0[0] / hw - 1.0
    proj[1], proj[9], proj[13] = -M[1, 0] / (step * hh), -M[1, 1] / (step * hh), 1.0 - t0[1] / hh
    proj[14], proj[15] = 0.5, 1.0
    u = np.zeros(44, np.float32)
    u[0:16] = np.eye(4, dtype=np.float32).ravel()
    u[16:32] = proj.astype(np.float32)
    u[32:36] = (0.5, 1.0, 0.3, 1.0)                        # sun, exposure
    u[36:39] = (1.0, 1.0, 0.0)                             # spacing, h_range, exaggeration 0
    return u


def lattice_fixed(cell, name):
    """The lattice in 24.8 fixed point: (X, Y) int64 arrays [j, i] -- what the snapped vertices must be."""
    n, M, t = lattice(cell, name)
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    P = np.stack([M[0, 0] * i + M[0, 1] * j + t[0], M[1, 0] * i + M[1, 1] * j + t[1]])
    F = P * 256.0
    assert np.array_equal(F, np.rint(F))
    return F[0].astype(np.int64), F[1].astype(np.int64)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def snapped_vertices(u, n):
    """The vertex stage of DESIGN.md section 4 restated in float32 for exaggeration 0 (h * 0 = 0 whatever the height): grid
    coordinate, view, projection, viewport, 24.8 snap.  Returns int64 (X, Y) arrays [j, i]."""
    f = np.float32
    assert u[38] == 0.0
    step = f(3.0) / (f(n) - f(1.0))
    g = f(-1.5) + np.arange(n, dtype=np.float32) * step
    x, z = np.meshgrid(g, g)
    x = x * max(u[36], f(1e-8)); z = z * max(u[36], f(1e-8))
    y, one = np.zeros_like(x), np.ones_like(x)

    def mat_vec(m, v):
        out = []
        for k in range(4):
            acc = m[k] * v[0]
            for c in (1, 2, 3):
                acc = _fma32(np.broadcast_to(m[4 * c + k], acc.shape), v[c], acc)
            out.append(acc)
        return out
    cp = mat_vec(u[16:32], mat_vec(u[0:16], [x, y, z, one]))
    assert np.all(cp[3] == 1.0) and np.all(cp[2] == 0.5)
    hw, hh = f(0.5 * W), f(0.5 * H)
    xf = _fma32(cp[0], np.broadcast_to(hw, x.shape), np.broadcast_to(hw, x.shape))
    yf = _fma32(-cp[1], np.broadcast_to(hh, x.shape), np.broadcast_to(hh, x.shape))
    return np.rint(xf * f(256.0)).astype(np.int64), np.rint(yf * f(256.0)).astype(np.int64)


def integer_visibility(X, Y):
    """Primitive id + 1 of the LAST front-facing triangle that covers each pixel centre, 0 for none: the coverage rule of DESIGN.md
    section 4 (edge functions on 24.8 integers, top-left rule) evaluated in int64 for every primitive of the grid in index order
    [a, c, b], [b, c, d] (a = (i, j), b = (i + 1, j), c = (i, j + 1), d = (i + 1, j + 1); id = 2 (j (n - 1) + i) + odd)."""
    n = X.shape[0]
    V = np.stack([X, Y], axis=-1)
    a, b, c, d = V[:-1, :-1], V[:-1, 1:], V[1:, :-1], V[1:, 1:]
    tris = np.stack([np.stack([a, c, b], axis=2), np.stack([b, c, d], axis=2)], axis=2).reshape(-1, 3, 2)     # [prim, vertex, xy]
    ids = np.arange(1, tris.shape[0] + 1, dtype=np.int64)
    x0 = np.maximum((tris[:, :, 0].min(axis=1) + 127) >> 8, 0); x1 = np.minimum((tris[:, :, 0].max(axis=1) - 128) >> 8, W - 1)
    y0 = np.maximum((tris[:, :, 1].min(axis=1) + 127) >> 8, 0); y1 = np.minimum((tris[:, :, 1].max(axis=1) - 128) >> 8, H - 1)
    keep = (x0 <= x1) & (y0 <= y1)
    tris, ids, x0, x1, y0, y1 = tris[keep], ids[keep], x0[keep], x1[keep], y0[keep], y1[keep]
    vis = np.zeros((H, W), np.int64)
    if not len(ids):
        return vis.astype(np.uint32)
    kx, ky = int((x1 - x0).max()) + 1, int((y1 - y0).max()) + 1
    oy, ox = np.meshgrid(np.arange(ky), np.arange(kx), indexing="ij")
    px = x0[:, None] + ox.ravel()[None, :]; py = y0[:, None] + oy.ravel()[None, :]
    inside = (px <= x1[:, None]) & (py <= y1[:, None])
    Px, Py = px * 256 + 128, py * 256 + 128
    area2 = (tris[:, 1, 0] - tris[:, 0, 0]) * (tris[:, 2, 1] - tris[:, 0, 1]) - (tris[:, 1, 1] - tris[:, 0, 1]) * (tris[:, 2, 0] - tris[:, 0, 0])
    inside &= (area2 < 0)[:, None]                         # front-facing = negative area in y-down pixels
    for e in range(3):
        va, vb = tris[:, (e + 1) % 3], tris[:, (e + 2) % 3]
        A, B = vb[:, 1] - va[:, 1], -(vb[:, 0] - va[:, 0])
        w = A[:, None] * (Px - va[:, 0:1]) + B[:, None] * (Py - va[:, 1:2])
        tl = (A > 0) | ((A == 0) & (B > 0))
        inside &= (w > 0) | ((w == 0) & tl[:, None])
    np.maximum.at(vis, (py[inside], px[inside]), np.broadcast_to(ids[:, None], px.shape)[inside])
    return vis.astype(np.uint32)


def lattice_coordinates(cell, name):
    """(i, j) float arrays [H, W]: the lattice coordinates of every pixel centre (exact: M's inverse is an integer matrix / cell)."""
    n, M, t = lattice(cell, name)
    yy, xx = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    Mi = np.linalg.inv(M)
    return Mi[0, 0] * (xx - t[0]) + Mi[0, 1] * (yy - t[1]), Mi[1, 0] * (xx - t[0]) + Mi[1, 1] * (yy - t[1])
