"""The cases of tests/test_gpu_limits.py are what they claim (tests/limit_cases.py): the oracle and the models alone, no GPU, show that
every case reaches the edge it is named for -- the first and the last tile column or row of a 16384-pixel frame, the last tile row and
both outer tile columns of the full frame's compared bands, 256 stripes with non-adjacent owners, partly occluded fields (the ambient
cases: tests/test_ambient_model.py), a NaN texel in the last column of a 32768-texel texture, millions of contour segments within and
beyond the record budget.  The soak corners at the frame limit are held the same way in tests/test_feature_soak_cases.py."""
import os

import numpy as np
import pytest

import limit_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
import support  # noqa: F401  (the repository root and the model directories on sys.path)


def outer_tiles(cov):
    """coverage (H, W) bool -> (the first, the last) tile column of a wide frame or tile row of a tall one"""
    H, W = cov.shape
    if W >= H:
        return cov[:, :lc.TILE], cov[:, lc.TILE * ((W - 1) // lc.TILE):]
    return cov[:lc.TILE], cov[lc.TILE * ((H - 1) // lc.TILE):]


def vis_of(c, oracle, luts, camera=None):
    u = lc.uniforms(c if camera is None else dict(c, camera=camera), oracle)
    return oracle.render_terrain(u, c["W"], c["H"], c["grid"], lc.heights(c), luts[c["cmap"]], nthreads=8)[1]


def test_the_constants_are_the_librarys():
    """the two limits the sources state as constants; the others are held by the refusals of 16385 pixels, 32769 texels, 257 stripes
    and an over-budget contour layer in the GPU tests"""
    root = os.path.dirname(HERE)
    assert f"kMaxStripes = {lc.MAX_STRIPES}" in open(os.path.join(root, "vulkan_forge_amd", "csrc", "vf_hip.hip")).read()
    assert f"#define VF_AMBIENT_REACH_MAX {lc.MAX_REACH}" in open(os.path.join(root, "include", "vf_hip.h")).read()


@pytest.mark.parametrize("case", lc.ASPECT_CASES + [lc.SHARD_WIDE, lc.SHARD_TALL], ids=lambda c: c["name"])
def test_every_frame_case_reaches_its_first_and_last_tile_and_covers_the_frame(oracle, luts, case):
    W, H = case["W"], case["H"]
    assert max(W, H) >= 16383 or (W, H) == (4097, 257)
    assert 129 <= case["grid"] <= 1025
    cov = vis_of(case, oracle, luts) != 0
    first, last = outer_tiles(cov)
    assert first.any() and last.any()
    assert cov.mean() >= 0.3
    if case["name"].endswith("grazing"):                       # the near plane cuts the frame: the same camera without it covers more
        whole = vis_of(case, oracle, luts, lc.uncut(case["camera"])) != 0
        assert whole.sum() > cov.sum() + 0.01 * cov.size
    elif case in lc.ASPECT_CASES:
        # Looking down, a primitive is as small as the grids of 129..1025 allow: the long side shows about 0.625 of the grid's cells, so a
        # cell is `cell` pixels wide (25.6 at grid 1025) and a primitive covers at most a cell clipped to the short side; 1.3 for the
        # parts of the surface that are up to 0.75 nearer to the eye than height 0 ((6 / 5.25)^2).  Measured 126-387 pixels a primitive:
        # a few pixels ACROSS in the 1- and 24-row frames, about 25 x 25 / 2 in the others; smaller needs a grid beyond 1025.
        ids = np.unique(vis_of(case, oracle, luts))
        cell = max(W, H) / (0.625 * (case["grid"] - 1))
        assert cov.sum() / max(len(ids) - 1, 1) < 1.3 * cell * min(cell, min(W, H)), cell


def test_the_aspect_cases_are_the_frames_the_limits_ask_for():
    sizes = {(c["W"], c["H"]) for c in lc.ASPECT_CASES}
    assert sizes == {(16384, 1), (16384, 24), (16383, 130), (1, 16384), (24, 16384), (130, 16383), (4097, 257)}
    assert all(sum(c["W"] == W and c["H"] == H for c in lc.ASPECT_CASES) == 2 for W, H in sizes)       # two cameras each
    fed = [c for c in lc.ASPECT_CASES if c["frames"] >= 3]
    assert any(c["W"] > c["H"] for c in fed) and any(c["W"] < c["H"] for c in fed)


def test_the_full_frames_compared_bands_hold_covered_pixels_in_the_outer_tiles(oracle, luts):
    c = lc.FULL
    W, H = c["W"], c["H"]
    assert (W, H, c["grid"], c["frames"]) == (lc.MAX_FRAME, lc.MAX_FRAME, 2049, 2)
    # more than 4096 tiles hold work (one run of the plan's sort): the same camera at a sixteenth of the size, where a tile is 4 x 4 pixels
    small = oracle.render_terrain(lc.uniforms(dict(c, W=W // 16, H=H // 16), oracle), W // 16, H // 16, c["grid"], lc.heights(c), luts[c["cmap"]], nthreads=8)[1] != 0
    assert int(small.reshape(H // 64, 4, W // 64, 4).any(axis=(1, 3)).sum()) > 4096
    u, h = lc.uniforms(c, oracle), lc.heights(c)
    col0 = col255 = row255 = False
    for rank in lc.FULL_RANKS:
        _, vis = oracle.render_terrain(u, W, H, c["grid"], h, luts[c["cmap"]], rank=rank, nranks=lc.FULL_NRANKS, band_h=lc.FULL_BAND, nthreads=8)
        rows = lc.rows_of(rank, lc.FULL_NRANKS, lc.FULL_BAND, H)
        cov = vis[rows] != 0                                   # (the oracle touches the rank's rows only)
        col0 |= bool(cov[:, :lc.TILE].any())
        col255 |= bool(cov[:, 255 * lc.TILE:].any())
        row255 |= bool((vis[255 * lc.TILE:] != 0).any()) if rows[-1] == H - 1 else False
        assert cov.mean() >= 0.3
    assert col0 and col255 and row255
    assert lc.rows_of(0, lc.FULL_NRANKS, lc.FULL_BAND, H)[0] == 0 and lc.rows_of(127, lc.FULL_NRANKS, lc.FULL_BAND, H)[-1] == H - 1


def test_the_stripe_map_is_uneven_and_deals_non_adjacent_stripes():
    owner = lc.stripe_owners()
    assert len(owner) == lc.MAX_STRIPES == lc.SHARD_WIDE["W"] // lc.TILE and owner.dtype == np.uint8
    counts = np.bincount(owner, minlength=lc.SHARD_RANKS)
    assert (counts > 0).all() and counts.max() >= 2 * counts.min()
    for r in range(lc.SHARD_RANKS):
        mine = np.flatnonzero(owner == r)
        assert (np.diff(mine) > 1).any(), r
    assert lc.SHARD_TALL["H"] // 64 == 256


@pytest.mark.parametrize("shape", lc.TEXTURE_SHAPES)
def test_the_big_textures_reach_32768_with_a_nan_texel_in_the_last_column_that_shows(oracle, luts, shape):
    h = lc.big_texture(shape)
    assert max(shape) == lc.MAX_TEXTURE and int(np.isnan(h).sum()) == 1 and np.isnan(h[:, -1]).any()
    W, H, G = lc.TEXTURE_FRAME
    u = oracle.default_uniforms(1, W, H)
    lut = luts["terrain"]
    vis = oracle.render_terrain(u, W, H, G, h, lut, nthreads=8)[1]
    assert (vis != 0).mean() > 0.05
    if shape[1] == lc.MAX_TEXTURE:                             # the grid samples one texel in 128: the last column is one of them
        clean = np.where(np.isnan(h), np.float32(0.0), h)
        assert not np.array_equal(oracle.render_terrain(u, W, H, G, clean, lut, nthreads=8)[1], vis)
        # and the two shade modes differ: SPEC_T32's texture normals matter
        a = oracle.render_terrain(u, W, H, G, h, lut, nthreads=8)[0]
        b = oracle.render_terrain(u, W, H, G, h, lut, nthreads=8, shade_mode=oracle.SHADE_SPEC_T32)[0]
        assert not np.array_equal(a, b)


def test_the_contour_case_has_millions_of_segments_within_the_budget_and_grid_33_beyond_it(oracle):
    import contour_model as cm
    c = lc.CONTOURS
    h, u = lc.heights(c), lc.uniforms(c, oracle)
    for grid, fits in ((c["grid"], True), (lc.CONTOURS_REFUSED_GRID, False)):
        levels = lc.contour_levels(cm.bounds(cm.surface(h, grid)))
        assert len(levels) == lc.MAX_LEVELS and (np.diff(levels) > 0).all() and np.isfinite(levels).all()
        L = cm.Layers()
        L.contours(h, grid, u, levels, width_px=1.0, rgba=(0, 0, 0, 255), join="round")
        assert len(L.recs[-1]) == 2 * L.nsegments
        if fits:
            assert 2000000 < L.nsegments < (1 << 23) and 2 * L.nsegments <= lc.RECORD_BUDGET
        else:
            assert 2 * L.nsegments > lc.RECORD_BUDGET
