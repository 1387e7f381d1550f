"""ctypes loader of the flood CPU model (flood_model.c).

    F = fdm.field_heights(h, level, seeds=None | "edges" | [(i, j), ...])       # h: (n, n) vertex heights; seeds: vertices
    F = fdm.field(uniforms, height, grid, level, seeds=None | "edges" | [(x, z), ...])   # the renderer's own surface; seeds: world (x, z)
    frame, d = fdm.frame(rgba, vis, uniforms, height, grid, F, shallow_rgba=..., deep_rgba=..., depth_full=0.1)
    flooded, passes = fdm.tile_passes(F.wet, fdm.sources(F.wet, seeds))         # the kernels' tile passes, emulated in numpy

F is a Field: .depth (n, n) float32 (the public field), .flooded and .wet (n, n) bool, .wd (n, n) float32, .vertices (the seeds'
vertices, (N, 2), or None).  `rgba` is the frame without water (H, W, 4) and `vis` its visibility (H, W) uint32; `d` (H, W) float32 is
each blended pixel's interpolated depth, -1 where the pass leaves the pixel.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import contour_model as cm
import model_support as ms
import overlay_model as om  # noqa: F401  (tests reach it as fdm.om)
import viewshed_model as vsm

TILE = 64
EVERYWHERE, EDGES, SEEDS = 0, 1, 2
DEFAULT_SHALLOW, DEFAULT_DEEP, DEFAULT_DEPTH_FULL = (96, 176, 224, 128), (16, 64, 160, 224), 0.1
Field = namedtuple("Field", "depth flooded wet wd vertices")

SIGNATURES = {
    "fdm_field": "i64(u8*, u8*, f32*, f32*, f32*, u32, f32, i32, u32*?, u32)",
    "fdm_label_tiles": "i64(i32*, u8*, u32, u32)",
    "fdm_frame": "i32(u8*, f32*, u32*, u32, u32, f32*, f32*, u32, u32, u32, u8*, f32*, u32, u32, f32)",
}


def lib():
    return ms.load("flood_model", SIGNATURES)


def mode_of(seeds):
    return EVERYWHERE if seeds is None else EDGES if isinstance(seeds, str) and seeds == "edges" else SEEDS


def seed_vertices(seeds, spacing, n):
    """(N, 2) world (x, z) of the overlays' frame -> (N, 2) uint32 vertices (i, j), each snapped as the viewshed's observer is"""
    return np.array([vsm.observer_vertex(s, spacing, n) for s in np.asarray(seeds, np.float32).reshape(-1, 2)], np.uint32).reshape(-1, 2)


def field_heights(h, level, seeds=None):
    """h (n, n) float32 vertex heights (row = z index, column = x index), seeds None / "edges" / vertices (i, j) -> Field"""
    h = np.ascontiguousarray(h, np.float32)
    n = h.shape[0]
    assert h.shape == (n, n)
    mode = mode_of(seeds)
    ij = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 2) if mode == SEEDS else None
    wet, fl = np.empty((n, n), np.uint8), np.empty((n, n), np.uint8)
    wd, depth = np.empty((n, n), np.float32), np.empty((n, n), np.float32)
    got = lib().fdm_field(wet, fl, wd, depth, h, n, float(np.float32(level)), mode, ij, len(ij) if ij is not None else 0)
    assert got == int(fl.sum()) and got >= 0
    return Field(depth, fl.astype(bool), wet.astype(bool), wd, ij)


def field(uniforms, height, grid, level, seeds=None):
    """the field of the renderer's surface; seeds in world (x, z) snap at the uniforms' spacing (u[36], at least 1e-8)"""
    n = max(int(grid), 2)
    if mode_of(seeds) == SEEDS:
        seeds = seed_vertices(seeds, cm.spacing_of(uniforms), n)
    return field_heights(cm.surface(height, grid), level, seeds)


def sources(wet, seeds):
    """the sources of a mode as an (n, n) bool array (not yet restricted to wet-able vertices)"""
    n = wet.shape[0]
    src = np.zeros((n, n), bool)
    mode = mode_of(seeds)
    if mode == EVERYWHERE:
        src[:] = True
    elif mode == EDGES:
        src[0, :] = src[-1, :] = src[:, 0] = src[:, -1] = True
    else:
        for i, j in np.asarray(seeds, np.int64).reshape(-1, 2):
            src[j, i] = True
    return src


def label_tiles(wet, tile=TILE):
    """(n, n) int32: 0 where not wet-able, else the number of the vertex's 4-connected component inside its tile"""
    w = np.ascontiguousarray(wet, np.uint8)
    lab = np.empty(w.shape, np.int32)
    assert lib().fdm_label_tiles(lab, w, w.shape[0], tile) >= 0
    return lab


def tile_passes(wet, src, tile=TILE):
    """The launches of k_flood_pass, emulated with Jacobi halos: in every pass each tile takes the border bits its four neighbours held
    BEFORE the pass, then runs to its own fixpoint (every component of the tile that holds a flooded bit floods).  -> (flooded, passes),
    passes counting up to and including the first pass that changed nothing.  The kernels may see a neighbour's stores of the same
    launch, so they never need more passes than this."""
    wet = np.asarray(wet, bool)
    n = wet.shape[0]
    lab = label_tiles(wet, tile)
    nlab = int(lab.max()) + 1
    fl = np.asarray(src, bool) & wet
    idx = np.arange(n)
    first, last = idx % tile == 0, idx % tile == tile - 1
    passes = 0
    while True:
        passes += 1
        halo = np.zeros((n, n), bool)
        halo[:, 1:] |= fl[:, :-1] & first[None, 1:]           # bit 63 of the left tile's row
        halo[:, :-1] |= fl[:, 1:] & last[None, :-1]           # bit 0 of the right tile's row
        halo[1:, :] |= fl[:-1, :] & first[1:, None]           # the last row of the tile above
        halo[:-1, :] |= fl[1:, :] & last[:-1, None]           # the first row of the tile below
        start = fl | (wet & halo)
        hit = np.zeros(nlab, bool)
        hit[lab[start]] = True
        hit[0] = False
        new = hit[lab]
        if np.array_equal(new, fl):
            return fl, passes
        fl = new


def tiles_reached(flooded, tile=TILE):
    """(tiles with a flooded vertex, tiles of the grid)"""
    n = flooded.shape[0]
    nt = (n + tile - 1) // tile
    return sum(bool(flooded[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile].any()) for ty in range(nt) for tx in range(nt)), nt * nt


def frame(rgba, vis, uniforms, height, grid, F, shallow_rgba=DEFAULT_SHALLOW, deep_rgba=DEFAULT_DEEP, depth_full=DEFAULT_DEPTH_FULL):
    """-> (the frame with the water (H, W, 4) uint8, d (H, W) float32)"""
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    d = np.empty(vis.shape, np.float32)
    assert lib().fdm_frame(out, d, vis, *scene, grid, np.ascontiguousarray(F.flooded, np.uint8), ms.field(F.wd), ms.pack(shallow_rgba),
                           ms.pack(deep_rgba), float(depth_full)) == 0
    return out, d


# ---- the inputs the GPU tests use (tests/test_gpu_flood.py), stated here so that tests/test_flood_model.py can hold them to the
# conditions that keep the comparisons from being vacuous ----

FIELD_TEXTURE = dict(seed=4, shape=(97, 131))                  # overlay_scenes.heights(4, (97, 131))
FIELD_GRIDS = (64, 65, 130, 203, 257)
FIELD_QUANTILES = (0.5, 0.45, 0.6)                             # the level: this quantile of the surface
SEED_VERTEX = (3, 3)


# The frame tests' scene (overlay_scenes.heights() on GRID vertices) is white noise of +-0.3 on four-vertex plateaus over the smooth
# analytic relief of +-0.5: below this level (the 0.43 quantile of the surface) lie the valleys of the relief, speckled with dry plateaus, and ponds on its slopes: three quarters of it flood.  Water
# from the border, and water from three seeds (one of them on a hill: no source).
SCENE_LEVEL = 0.1
SCENE_SEEDS = ("edges", [(-1.2, -1.3), (0.9, 1.1), (0.1, -0.2)])


def vertex_xz(v, n, spacing=1.0):
    """the world (x, z) of vertex (i, j)"""
    step = np.float32(3.0) / np.float32(n - 1)
    return tuple(float((np.float32(-1.5) + np.float32(k) * step) * np.float32(spacing)) for k in v)


def field_level(h, q=0.5):
    return float(np.float32(np.quantile(h.astype(np.float64), q)))


def field_seed_lists(h, level, n):
    """world-frame seed lists of the field cases: the one seed; and the list -- the seed, a seed on dry ground, the seed again, and a
    seed far outside the grid (clamped to the border)"""
    one = [vertex_xz(SEED_VERTEX, n)]
    dry = np.argwhere(~(h < level))[0]                         # (j, i) of the first vertex that is not wet-able
    return one, [one[0], vertex_xz((int(dry[1]), int(dry[0])), n), one[0], (9.0, -0.2)]


def serpentine(n=130, wall=1.0, floor=-1.0):
    """A texture the size of the grid (n x n): floor corridors one vertex wide along the rows j = 1, 3, 5, ..., walls between them, each
    wall open at alternating ends -- one channel that runs the width of the grid back and forth and crosses every tile border of a row
    of tiles in each corridor.  -> (texture, the channel's first vertex (i, j), its number of vertices)"""
    t = np.full((n, n), wall, np.float32)
    rows = list(range(1, n - 1, 2))
    for k, j in enumerate(rows):
        t[j, 1:n - 1] = floor
        if k + 1 < len(rows):
            t[j + 1, n - 2 if k % 2 == 0 else 1] = floor
    return t, (1, 1), int((t == floor).sum())
