"""The flood CPU model (tests/flood_model) against what a flood must do: a hand-worked basin with a dike and a diagonal
gap that must not leak; monotone in the level; the flood of a seed list is the union of the single floods; dry, duplicate and clamped
seeds; non-finite vertices block; the eight symmetries of the square; `edges` and `everywhere` against their definitions; the tile
passes of the kernels, emulated in numpy, equal the search; a hand-worked tinted pixel; and the inputs of the GPU tests
(tests/test_gpu_flood.py) meet the conditions that keep those comparisons from being vacuous."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
from support import bits, smooth
import flood_model as fdm
from overlay_scenes import CAMERAS, GRID, heights

cm = fdm.cm


def vertices(mask):
    """the set of (i, j) of a (j, i) bool array"""
    return {(int(i), int(j)) for j, i in np.argwhere(mask)}


# ---- items 1-4: the field ----

BASIN = np.array([[1, 1, 1, 1, 1],
                  [1, 0, 1, 0, 1],
                  [1, 0, 1, 1, 1],
                  [1, 0, 0, 1, 0],
                  [1, 1, 1, 0, 1]], np.float32)                # [j][i]; 0: below the level 0.5


def test_a_hand_worked_basin_with_a_dike_and_a_diagonal_gap():
    """Seven vertices lie below the level.  From (1, 1) the water runs down column 1 and round the corner to (2, 3).  (3, 1) lies behind
    the dike of column 2; (3, 4) touches (2, 3) only by a corner, (4, 3) touches (3, 4) only by a corner: neither is reached."""
    wet = {(1, 1), (3, 1), (1, 2), (1, 3), (2, 3), (4, 3), (3, 4)}
    F = fdm.field_heights(BASIN, 0.5, [(1, 1)])
    assert vertices(F.wet) == wet
    assert vertices(F.flooded) == {(1, 1), (1, 2), (1, 3), (2, 3)}
    assert np.array_equal(F.depth, np.where(F.flooded, np.float32(0.5), np.float32(0.0)))
    assert np.array_equal(F.wd, np.float32(0.5) - BASIN) and (F.wd[~F.wet] == -0.5).all()      # wd is signed
    assert vertices(fdm.field_heights(BASIN, 0.5, [(3, 4)]).flooded) == {(3, 4)}
    assert vertices(fdm.field_heights(BASIN, 0.5, [(2, 2)]).flooded) == set()               # a seed on the dike is no source
    assert vertices(fdm.field_heights(BASIN, 0.5, "edges").flooded) == {(4, 3), (3, 4)}     # the wet-able border vertices, and no further
    assert vertices(fdm.field_heights(BASIN, 0.5, None).flooded) == wet
    assert vertices(fdm.field_heights(BASIN, 1.0, None).flooded) == wet                     # h < level is strict: 1 is not below 1
    assert vertices(fdm.field_heights(BASIN, 1.5, [(1, 1)]).flooded) == vertices(np.ones((5, 5), bool))
    assert vertices(fdm.field_heights(BASIN, 0.0, None).flooded) == set()                   # ... and 0 is not below 0


def test_the_flood_grows_with_the_level():
    h = smooth(97, 5)
    last = np.zeros(h.shape, bool)
    grew = 0
    for q in (0.2, 0.35, 0.5, 0.65, 0.8):
        F = fdm.field_heights(h, np.quantile(h, q), [(40, 40), (3, 90)])
        assert not (last & ~F.flooded).any(), q
        grew += int((F.flooded & ~last).any())
        last = F.flooded
    assert grew >= 3 and not last.all()


def test_the_flood_of_a_seed_list_is_the_union_of_the_single_floods():
    h = heights(2, (40, 40))
    h = cm.surface(h, 90)
    level = fdm.field_level(h, 0.55)
    seeds = [(3, 3), (80, 10), (45, 45), (10, 85), (88, 88)]
    singles = [fdm.field_heights(h, level, [s]).flooded for s in seeds]
    union = np.logical_or.reduce(singles)
    assert np.array_equal(fdm.field_heights(h, level, seeds).flooded, union)
    assert len({s.tobytes() for s in singles}) >= 2 and union.any() and not np.array_equal(union, fdm.field_heights(h, level, None).flooded)


def test_dry_duplicate_and_clamped_seeds():
    n = 65
    h = smooth(n, 8)
    level = fdm.field_level(h, 0.5)
    wet = h < level
    j, i = (int(v) for v in np.argwhere(wet)[0])
    dj, di = (int(v) for v in np.argwhere(~wet)[0])
    one = fdm.field_heights(h, level, [(i, j)])
    assert one.flooded[j, i] and not one.flooded.all()
    assert not fdm.field_heights(h, level, [(di, dj)]).flooded.any()                           # dry ground is no source
    assert np.array_equal(fdm.field_heights(h, level, [(i, j), (di, dj), (i, j)]).flooded, one.flooded)
    # world coordinates snap as the viewshed's observer does, and clamp to the border
    assert fdm.seed_vertices([(0.0, 0.0), (-1.5, 1.5), (9.0, -40.0)], 1.0, n).tolist() == [[32, 32], [0, 64], [64, 0]]
    assert fdm.seed_vertices([(3.0, -3.0)], 2.0, n).tolist() == [[64, 0]]                       # the overlays' frame: times spacing
    step = 3.0 / (n - 1)
    assert fdm.seed_vertices([(-1.5 + 10.4 * step, -1.5 + 10.6 * step)], 1.0, n).tolist() == [[10, 11]]
    assert fdm.vertex_xz((10, 11), n) == pytest.approx((-1.5 + 10 * step, -1.5 + 11 * step))
    u = np.zeros(44, np.float32)
    u[36] = 1.0
    tex = np.zeros((1, 1), np.float32)
    F = fdm.field(u, tex, n, 10.0, [(9.0, -40.0)])
    assert F.vertices.tolist() == [[64, 0]] and F.flooded.all()


def test_non_finite_vertices_block_and_are_never_wet():
    n = 33
    for bad in (np.nan, np.inf, -np.inf):
        h = np.zeros((n, n), np.float32)
        h[:, 16] = bad                                         # a wall of the bad value across the grid
        F = fdm.field_heights(h, 1.0, [(3, 3)])
        assert F.flooded[:, :16].all() and not F.flooded[:, 16:].any(), bad
        assert not F.wet[:, 16].any() and (F.depth[:, 16] == 0).all() and not np.isfinite(F.wd[:, 16]).any()
        h[20, 16] = 0.0                                        # one gap: the water gets through
        assert fdm.field_heights(h, 1.0, [(3, 3)]).flooded.sum() == n * n - (n - 1)
    assert not fdm.field_heights(np.full((5, 5), np.nan, np.float32), 1.0, None).flooded.any()


def test_the_field_commutes_with_the_eight_symmetries_of_the_square():
    n = 97
    h = smooth(n, 3)
    level = fdm.field_level(h, 0.5)
    for seeds in ([(0, 0)], [(96, 40), (13, 77)], "edges"):
        f = fdm.field_heights(h, level, seeds)
        for transpose in (False, True):
            for mi in (False, True):
                for mj in (False, True):
                    g, want = h, f.depth
                    v = seeds if isinstance(seeds, str) else list(seeds)
                    if transpose:
                        g, want = g.T, want.T
                        v = v if isinstance(v, str) else [(b, a) for a, b in v]
                    if mi:
                        g, want = g[:, ::-1], want[:, ::-1]
                        v = v if isinstance(v, str) else [(n - 1 - a, b) for a, b in v]
                    if mj:
                        g, want = g[::-1, :], want[::-1, :]
                        v = v if isinstance(v, str) else [(a, n - 1 - b) for a, b in v]
                    got = fdm.field_heights(np.ascontiguousarray(g), level, v)
                    assert np.array_equal(bits(got.depth), bits(want)), (seeds, transpose, mi, mj)
    assert fdm.field_heights(h, level, "edges").flooded.any()


def test_edges_and_everywhere_against_their_definitions():
    n = 90
    h = cm.surface(heights(6, (33, 47)), n)
    level = fdm.field_level(h, 0.5)
    wet = np.isfinite(h) & (h < level)
    every = fdm.field_heights(h, level, None)
    assert np.array_equal(every.flooded, wet) and np.array_equal(every.wet, wet)
    assert np.array_equal(bits(every.depth), bits(np.where(wet, np.float32(level) - h, np.float32(0))))
    border = [(i, j) for i in range(n) for j in range(n) if i in (0, n - 1) or j in (0, n - 1)]
    edges = fdm.field_heights(h, level, "edges")
    assert np.array_equal(edges.flooded, fdm.field_heights(h, level, border).flooded)
    assert edges.flooded.any() and (wet & ~edges.flooded).any()                              # (ponds inland stay dry)


# ---- the kernels' tile passes ----

@pytest.mark.parametrize("n", [64, 65, 130, 203])
def test_the_tile_pass_emulation_equals_the_search(n):
    h = cm.surface(heights(4, (97, 131)), n)
    h[n // 2, n // 3] = np.nan
    for q in (0.4, 0.5, 0.62):
        level = fdm.field_level(h, q)
        for seeds in ([(3, 3)], [(n - 1, n - 1), (n // 2, 5), (70 % n, 63)], "edges", None):
            F = fdm.field_heights(h, level, seeds)
            got, passes = fdm.tile_passes(F.wet, fdm.sources(F.wet, seeds))
            assert np.array_equal(got, F.flooded), (n, q, seeds)
            assert passes >= (1 if seeds is None or not F.flooded.any() else 2)


def test_the_serpentine_is_what_was_built_and_needs_many_passes():
    n = 130
    tex, start, count = fdm.serpentine(n)
    assert tex.shape == (n, n)
    h = cm.surface(tex, n)
    assert np.array_equal(h < 0.0, tex == -1.0) and np.isfinite(h).all()                     # a texture the size of the grid: one texel per vertex
    F = fdm.field_heights(h, 0.0, [start])
    assert np.array_equal(F.flooded, tex == -1.0) and int(F.flooded.sum()) == count          # one channel: all of it floods from its first vertex
    corridor = F.flooded[1, :]
    assert corridor[1:n - 1].all() and corridor[63] and corridor[64] and corridor[127] and corridor[128]   # it crosses the tile borders at 64 and 128
    assert F.flooded[2, n - 2] and not F.flooded[2, 1] and F.flooded[4, 1] and not F.flooded[4, n - 2]   # ... back and forth
    got, passes = fdm.tile_passes(F.wet, fdm.sources(F.wet, [start]))
    assert np.array_equal(got, F.flooded)
    assert passes >= 8, passes
    assert fdm.tiles_reached(F.flooded) == (6, 9)                                            # (the last row of tiles holds the rows 128 and 129: wall)


# ---- the conditions that keep the GPU comparisons from being vacuous ----

@pytest.mark.parametrize("n", fdm.FIELD_GRIDS)
def test_the_gpu_tests_field_cases_are_not_vacuous(n):
    """On every seeded field case the flooded share of the wet-able vertices lies strictly between 50 % and 95 %; from grid 65 on the
    flooded set reaches at least two tiles and the emulation needs at least 3 passes.  (Grid 64 is one whole tile: one tile is all it
    can reach, and its second pass is the one that changes nothing.)  `edges` leaves ponds dry and holds the same share; it reaches
    two tiles and needs 3 passes from grid 130 on only -- at grid 65 every tile has border vertices of its own and the emulation is
    done in 2 passes, so that case checks the sources and the masks, not the halos.  `everywhere` is the wet-able set, by definition
    without a pass."""
    tex = heights(**fdm.FIELD_TEXTURE)
    h = cm.surface(tex, n)
    u = np.zeros(44, np.float32)
    u[36] = 1.0
    for q in fdm.FIELD_QUANTILES:
        level = fdm.field_level(h, q)
        one, several = fdm.field_seed_lists(h, level, n)
        for seeds in (one, several):
            F = fdm.field(u, tex, n, level, seeds)
            assert F.vertices[0].tolist() == list(fdm.SEED_VERTEX)
            share = F.flooded.sum() / F.wet.sum()
            reached, of = fdm.tiles_reached(F.flooded)
            _, passes = fdm.tile_passes(F.wet, fdm.sources(F.wet, F.vertices))
            assert 0.5 < share < 0.95, (n, q, share)
            if n > 64:
                assert reached >= 2 and passes >= 3, (n, q, reached, passes)
            else:
                assert (reached, of, passes) == (1, 1, 2)
        assert len(several) == 4 and several[0] == several[2]
        v = fdm.field(u, tex, n, level, several).vertices
        assert not (h[v[1, 1], v[1, 0]] < level) and v[3, 0] == n - 1                        # a dry seed, and one clamped to the border
        edges = fdm.field(u, tex, n, level, "edges")
        assert 0.5 < edges.flooded.sum() / edges.wet.sum() < 0.95
        reached, _ = fdm.tiles_reached(edges.flooded)
        _, passes = fdm.tile_passes(edges.wet, fdm.sources(edges.wet, "edges"))
        if n >= 130:
            assert reached >= 2 and passes >= 3, (n, q, reached, passes)
        else:
            assert passes == 2, (n, q, passes)
        assert np.array_equal(fdm.field(u, tex, n, level, None).flooded, np.isfinite(h) & (h < level))


def test_the_table_of_the_design():
    """level at the median, one seed at vertex (3, 3)"""
    tex = heights(**fdm.FIELD_TEXTURE)
    want = {130: (6548, 8450, 6, 9, 6), 203: (15850, 20604, 9, 16, 6), 257: (25418, 33024, 13, 25, 9)}
    for n, row in want.items():
        h = cm.surface(tex, n)
        F = fdm.field_heights(h, fdm.field_level(h), [fdm.SEED_VERTEX])
        _, passes = fdm.tile_passes(F.wet, fdm.sources(F.wet, [fdm.SEED_VERTEX]))
        assert (int(F.flooded.sum()), int(F.wet.sum()), *fdm.tiles_reached(F.flooded), passes) == row, n


# ---- item 5: the frame ----

def python_pixel(rgba, d, shallow, deep, depth_full):
    """contract item 5 from the interpolated depth on, in numpy binary32"""
    f = np.float32
    s = min(f(d) / f(depth_full), f(1.0))
    c = [f(fdm.om.lib().ovm_decode(int(v))) for v in rgba[:3]]
    for col, cov in ((shallow, f(1.0) - s), (deep, s)):
        a = f(cov) * (f(col[3]) / f(255.0))
        if a > 0:
            c = [f(fdm.om.lib().ovm_decode(int(col[k]))) * a + c[k] * (f(1.0) - a) for k in range(3)]
    return [int(fdm.om.lib().ovm_encode(float(v))) for v in c] + [255]


def test_a_hand_worked_tinted_pixel():
    """Water 0.05 deep everywhere under depth_full 0.1: s = 0.5 (to rounding), the shallow colour with coverage 0.5, then the deep one
    with coverage 0.5, over the frame's own colour, in linear light."""
    import oracle
    W, H, n = 96, 64, 33
    tex = np.zeros((1, 1), np.float32)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), np.float32).reshape(44)
    lut = np.load(os.path.join(HERE, "golden", "colormaps_rgba8.npz"))["viridis"]
    rgba, vis = oracle.render_terrain(u, W, H, n, tex, lut, want_vis=True, nthreads=4)
    rgba = rgba.reshape(H, W, 4)
    flooded = np.ones((n, n), bool)
    F = fdm.Field(None, flooded, flooded, np.full((n, n), 0.05, np.float32), None)
    shallow, deep = (96, 176, 224, 128), (16, 64, 160, 224)
    out, d = fdm.frame(rgba, vis, u, tex, n, F, shallow, deep, 0.1)
    covered = vis != 0
    assert covered.any() and (~covered).any()
    assert (d[~covered] == -1).all() and np.array_equal(out[~covered], rgba[~covered])
    assert np.abs(d[covered] - 0.05).max() <= 1e-7                       # a constant interpolates to itself, to an ulp
    py, px = (int(v) for v in np.argwhere(covered)[covered.sum() // 2])
    assert out[py, px].tolist() == python_pixel(rgba[py, px], d[py, px], shallow, deep, 0.1)
    assert out[py, px].tolist() != rgba[py, px].tolist()
    for y, x in np.argwhere(covered)[::37]:
        assert out[y, x].tolist() == python_pixel(rgba[y, x], d[y, x], shallow, deep, 0.1), (x, y)
    # the cases that leave the pixel as drawn: no flooded vertex; a non-finite wd; d not > 0; colours without alpha
    dry = fdm.Field(None, np.zeros((n, n), bool), flooded, F.wd, None)
    assert np.array_equal(fdm.frame(rgba, vis, u, tex, n, dry, shallow, deep, 0.1)[0], rgba)
    nan = fdm.Field(None, flooded, flooded, np.full((n, n), np.nan, np.float32), None)
    assert np.array_equal(fdm.frame(rgba, vis, u, tex, n, nan, shallow, deep, 0.1)[0], rgba)
    neg = fdm.Field(None, flooded, flooded, np.full((n, n), -0.05, np.float32), None)
    assert np.array_equal(fdm.frame(rgba, vis, u, tex, n, neg, shallow, deep, 0.1)[0], rgba)
    assert np.array_equal(fdm.frame(rgba, vis, u, tex, n, F, (1, 2, 3, 0), (4, 5, 6, 0), 0.1)[0], rgba)
    # deeper than depth_full: the deep colour alone (coverage 1 - s = 0 writes nothing)
    deep_only, _ = fdm.frame(rgba, vis, u, tex, n, F, shallow, deep, 0.01)
    assert deep_only[py, px].tolist() == python_pixel(rgba[py, px], 1.0, (0, 0, 0, 0), deep, 1.0)


@pytest.mark.parametrize("size", [(640, 360), (257, 131)])
def test_the_gpu_tests_scene_is_part_under_water(size):
    """Every tinted frame of tests/test_gpu_flood.py changes some pixels and leaves some covered pixels alone."""
    import oracle
    W, H = size
    h = heights()
    lut = np.zeros(1024, np.uint8)
    for cam in CAMERAS:
        u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam]), np.float32).reshape(44)
        rgba, vis = oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True, nthreads=8)
        rgba = rgba.reshape(H, W, 4)
        covered = vis != 0
        for seeds in fdm.SCENE_SEEDS:
            F = fdm.field(u, h, GRID, fdm.SCENE_LEVEL, seeds)
            assert F.flooded.any() and (F.wet & ~F.flooded).any() and not F.wet.all()
            out, d = fdm.frame(rgba, vis, u, h, GRID, F)
            wetpx = d > 0
            frac = float(wetpx[covered].mean())
            assert 0.01 < frac < 0.99, (cam, size, seeds if isinstance(seeds, str) else "list", frac)
            assert not wetpx[~covered].any() and np.array_equal(out[~wetpx], rgba[~wetpx])
            assert (out[wetpx] != rgba[wetpx]).any()
