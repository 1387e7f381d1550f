"""ctypes loader of the spill CPU model (spill_model.c).

    F = spm.field_heights(h, seeds="edges" | [(i, j), ...])                      # h: (n, n) vertex heights; seeds: vertices
    F = spm.field(uniforms, height, grid, seeds="edges" | [(x, z), ...])         # the renderer's own surface; seeds: world (x, z)
    frame, d = spm.frame(rgba, vis, uniforms, height, grid, F, shallow_rgba=..., deep_rgba=..., depth_full=0.1)
    F2, passes, changed_tiles = spm.tile_passes(h, seeds)                        # the kernels' tile passes, emulated

F is a Field: .spill (n, n) float32 and .sink (n, n) float32 (the public fields), .sd (n, n) float32 (spill - h, not finite where either
is not), .reached (n, n) bool, .vertices (the seeds' vertices, (N, 2), or None).  `rgba` is the frame without the tint (H, W, 4) and
`vis` its visibility (H, W) uint32; `d` (H, W) float32 is each blended pixel's interpolated depth, -1 where the pass leaves the pixel.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import contour_model as cm
import flood_model as fdm
import model_support as ms

TILE = 64
EDGES, SEEDS = 1, 2
DEFAULT_SHALLOW, DEFAULT_DEEP, DEFAULT_DEPTH_FULL = (96, 176, 224, 128), (16, 64, 160, 224), 0.1
Field = namedtuple("Field", "spill sink sd reached vertices")

SIGNATURES = {
    "spm_key": "u32(f32)",
    "spm_unkey": "f32(u32)",
    "spm_field": "i64(f32*, f32*, f32*, f32*, u32, i32, u32*?, u32)",
    "spm_tile_passes": "i64(f32*, f32*, f32*, f32*, u32, i32, u32*?, u32, u32, u32*, u32)",
    "spm_frame": "i32(u8*, f32*, u32*, u32, u32, f32*, f32*, u32, u32, u32, f32*, u32, u32, f32)",
}


def lib():
    return ms.load("spill_model", SIGNATURES)


def mode_of(seeds):
    return EDGES if isinstance(seeds, str) and seeds == "edges" else SEEDS


def key(x):
    """the uint32 sort key of float32 array x (contract item 1), in numpy"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return b ^ np.where(b >> 31, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def key_min(a, b):
    """the minimum of two float32 arrays in key order"""
    return np.where(key(a) <= key(b), a, b).astype(np.float32)


def _args(h, seeds):
    h = np.ascontiguousarray(h, np.float32)
    n = h.shape[0]
    assert h.shape == (n, n)
    mode = mode_of(seeds)
    ij = np.ascontiguousarray(seeds, np.uint32).reshape(-1, 2) if mode == SEEDS else None
    out = [np.empty((n, n), np.float32) for _ in range(3)]
    return h, n, mode, ij, out


def field_heights(h, seeds="edges"):
    """h (n, n) float32 vertex heights (row = z index, column = x index), seeds "edges" / vertices (i, j) -> Field (the search)"""
    h, n, mode, ij, (spill, sd, sink) = _args(h, seeds)
    got = lib().spm_field(spill, sd, sink, h, n, mode, ij, len(ij) if ij is not None else 0)
    assert got >= 0
    reached = np.isfinite(spill)
    assert got == int(reached.sum())
    return Field(spill, sink, sd, reached, ij)


def tile_passes(h, seeds="edges", tile=TILE):
    """The launches of k_spill_pass, emulated with Jacobi halos -> (Field, passes, changed_tiles): passes counts up to and including the
    first pass that changed nothing, changed_tiles[p] is the number of tiles pass p + 1 changed."""
    h, n, mode, ij, (spill, sd, sink) = _args(h, seeds)
    cap = 4096
    changed = np.zeros(cap, np.uint32)
    passes = lib().spm_tile_passes(spill, sd, sink, h, n, mode, ij, len(ij) if ij is not None else 0, tile, changed, cap)
    assert 0 < passes <= cap
    return Field(spill, sink, sd, np.isfinite(spill), ij), int(passes), changed[:passes].copy()


def field(uniforms, height, grid, seeds="edges"):
    """the field of the renderer's surface; seeds in world (x, z) snap at the uniforms' spacing, as the flood's do"""
    n = max(int(grid), 2)
    if mode_of(seeds) == SEEDS:
        seeds = fdm.seed_vertices(seeds, cm.spacing_of(uniforms), n)
    return field_heights(cm.surface(height, grid), seeds)


def n_tiles(n, tile=TILE):
    return ((n + tile - 1) // tile) ** 2


def frame(rgba, vis, uniforms, height, grid, F, shallow_rgba=DEFAULT_SHALLOW, deep_rgba=DEFAULT_DEEP, depth_full=DEFAULT_DEPTH_FULL):
    """-> (the frame with the sink tint (H, W, 4) uint8, d (H, W) float32)"""
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    d = np.empty(vis.shape, np.float32)
    assert lib().spm_frame(out, d, vis, *scene, grid, ms.field(F.sd), ms.pack(shallow_rgba), ms.pack(deep_rgba), float(depth_full)) == 0
    return out, d


# ---- the inputs the GPU tests use (tests/test_gpu_spill.py), stated here so that tests/test_spill_model.py can hold them to the
# conditions that keep the comparisons from being vacuous ----

FIELD_TEXTURE = fdm.FIELD_TEXTURE                              # overlay_scenes.heights(4, (97, 131))
FIELD_GRIDS = fdm.FIELD_GRIDS                                  # (64, 65, 130, 203, 257)
FIELD_QUANTILES = fdm.FIELD_QUANTILES
SEED_VERTEX = fdm.SEED_VERTEX                                  # (3, 3)
vertex_xz = fdm.vertex_xz

# The frame tests' scene: water from the border, and from three seeds (the flood's: one of them on a hill)
SCENE_SEEDS = fdm.SCENE_SEEDS


def field_seed_lists(h, n):
    """world-frame seed lists of the field cases: the one seed; and the list -- the seed, a seed on a dry (non-passable) vertex when h
    has one (else the seed's neighbour), the seed again, and a seed far outside the grid (clamped to the border)"""
    one = [vertex_xz(SEED_VERTEX, n)]
    dry = np.argwhere(~np.isfinite(h))
    other = (int(dry[0][1]), int(dry[0][0])) if len(dry) else (SEED_VERTEX[0] + 1, SEED_VERTEX[1])
    return one, [one[0], vertex_xz(other, n), one[0], (9.0, -0.2)]


def dry_texture(tex):
    """the field cases' texture with a 3 x 3 block of NaN texels (every grid of FIELD_GRIDS samples it): the non-passable vertices the
    seed list's dry seed sits on"""
    g = np.array(tex, np.float32)
    g[40:43, 50:53] = np.nan
    return g


def serpentine(n=130, slope=+1.0):
    """flood_model.serpentine's channel with a floor that rises (slope > 0) or falls (slope < 0) along the channel from its first
    vertex; walls of 1.0, floor within [-1, -0.5].  -> (texture, the channel's first vertex (i, j))"""
    t, first, count = fdm.serpentine(n)
    rows = list(range(1, n - 1, 2))
    k = 0
    for r, j in enumerate(rows):
        cols = list(range(1, n - 1))
        if r % 2 == 1:
            cols.reverse()
        for i in cols:
            t[j, i] = np.float32(-0.75 + slope * 0.25 * (2.0 * k / count - 1.0)); k += 1
        if r + 1 < len(rows):
            t[j + 1, cols[-1]] = np.float32(-0.75 + slope * 0.25 * (2.0 * k / count - 1.0)); k += 1
    assert k == count
    return t, first
