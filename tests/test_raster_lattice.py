"""The lattice frames of tests/raster_lattice.py are what the GPU test (tests/test_gpu_raster_device.py) takes them for: every
grid vertex snaps exactly onto the half-pixel lattice (pixel centres for cells of 8 and 1 pixel), the lattice fills what it should
with front-facing triangles, and the oracle's primitive ids on it are those of the coverage rule evaluated on integers -- edges
and vertices through pixel centres, where only the top-left rule decides.  CPU only; a case that failed here would make its GPU
twin vacuous."""
import numpy as np
import pytest

import raster_lattice as rl


@pytest.fixture(scope="module")
def frames(oracle, luts):
    """The oracle's frame of every case, rendered once."""
    out = {}
    for cell, name in rl.CASES:
        u = rl.uniforms(cell, name)
        out[cell, name] = oracle.render_terrain(u, rl.W, rl.H, rl.GRID[cell], oracle.SPIKE_DUMMY_HEIGHT, luts["viridis"])
    return out


@pytest.mark.parametrize("cell,name", rl.CASES)
def test_vertices_snap_onto_pixel_centres(cell, name):
    n = rl.GRID[cell]
    X, Y = rl.snapped_vertices(rl.uniforms(cell, name), n)
    LX, LY = rl.lattice_fixed(cell, name)
    assert np.array_equal(X, LX) and np.array_equal(Y, LY)
    pitch = 256 if cell >= 1.0 else 128
    assert np.all((X - 128) % pitch == 0) and np.all((Y - 128) % pitch == 0)
    on_screen = (X > 0) & (X < rl.W * 256) & (Y > 0) & (Y < rl.H * 256)
    assert on_screen.any() and not on_screen.all()        # the lattice is partly off-screen
    centres = on_screen & ((X - 128) % 256 == 0) & ((Y - 128) % 256 == 0)
    assert centres.sum() >= 50                             # vertices ON pixel centres of the target
    # lattice lines cross the tile boundary (pixel 64) in both axes
    assert (X.min() < 64 * 256 < X.max()) and (Y.min() < 64 * 256 < Y.max())


@pytest.mark.parametrize("cell,name", rl.CASES)
def test_the_lattice_is_covered_inside_and_empty_outside(frames, cell, name):
    n = rl.GRID[cell]
    _rgba, vis = frames[cell, name]
    i, j = rl.lattice_coordinates(cell, name)
    inside = (i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)
    outside = (i < 0) | (i > n - 1) | (j < 0) | (j > n - 1)
    assert inside.sum() > 1000 and outside.sum() > 100
    assert np.all(vis[inside] != 0)
    assert np.all(vis[outside] == 0)


@pytest.mark.parametrize("cell,name", rl.CASES)
def test_oracle_ids_equal_the_integer_top_left_evaluation(frames, cell, name):
    _rgba, vis = frames[cell, name]
    X, Y = rl.lattice_fixed(cell, name)
    want = rl.integer_visibility(X, Y)
    assert np.array_equal(vis, want), f"{int((vis != want).sum())} pixels differ"
    # the rule is at work: pixel centres ON lattice lines are covered, each by exactly the triangle the rule names
    i, j = rl.lattice_coordinates(cell, name)
    n = rl.GRID[cell]
    on_line = ((i == np.rint(i)) | (j == np.rint(j)) | (i + j == np.rint(i + j))) & (i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)
    assert on_line.sum() > 500 and np.all(vis[on_line] != 0)
