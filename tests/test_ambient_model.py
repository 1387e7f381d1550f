"""The ambient-occlusion CPU model (tests/ambient_model) against what a sky-view factor must do: a numpy restatement of
the contract agrees bit for bit, the field commutes with the grid's mirrors and its transposition, does not know `strength`, is 1
on a plane and down a tilted one, a single step gives the hand-computed value, the reach is isotropic, and the scenes the GPU tests
draw are partly occluded."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
from support import bits, smooth
import ambient_model as abm
import shadow_model as shm
from overlay_scenes import CAMERAS, GRID, heights

f32 = np.float32
# general directions in every octant, the axes, exact diagonals
DIRS = np.array([(0.9, 0.31), (0.31, 0.9), (-0.31, 0.9), (-0.9, 0.31), (-0.9, -0.31), (-0.31, -0.9), (0.31, -0.9), (0.9, -0.31),
                 (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)], f32)


def brute_force(h, dirs, spacing, exag, reach):
    """the contract in numpy binary32, a whole grid and one distance m at a time"""
    n = h.shape[0]
    y = h * f32(exag)
    fin = np.isfinite(y)
    J, I = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")           # row = z index, column = x index
    step = (f32(2.0) * f32(1.5)) / (f32(n) - f32(1.0))
    acc = None
    with np.errstate(all="ignore"):
        for ux, uz in np.asarray(dirs, f32):
            zmajor = abs(uz) > abs(ux)
            smaj, smin = (uz, ux) if zmajor else (ux, uz)
            a = f32(abs(smin)) / f32(abs(smaj))
            s = -1 if smin < 0 else 1
            major, minor = (J, I) if zmajor else (I, J)
            k = n - 1 - major if smaj > 0 else major                        # steps count from the direction's side
            shear = np.rint(np.arange(n, dtype=f32) * a).astype(np.int64)
            c = minor + s * shear[k]                                        # the line's intercept
            g = fma_g(a)
            ell = (step * f32(spacing)) * g
            R = max(1, int(np.floor(f32(reach) / g)))
            T = np.zeros((n, n), f32)
            for m in range(1, min(R, n - 1) + 1):
                km = k - m
                ok = km >= 0
                mi = c - s * shear[np.where(ok, km, 0)]
                ok &= (mi >= 0) & (mi < n)
                ma = n - 1 - km if smaj > 0 else km
                jj, ii = (ma, mi) if zmajor else (mi, ma)
                y2 = y[np.where(ok, jj, 0), np.where(ok, ii, 0)]
                ok &= np.isfinite(y2)
                inv = f32(1.0) / (f32(m) * ell)
                term = (y2 - y) * inv
                T = np.where(ok & ~np.isnan(term) & (term > T), term, T)
            occ = np.where(fin, f32(1.0) - f32(1.0) / (f32(1.0) + T * T), f32(0.0)).astype(f32)
            acc = occ if acc is None else acc + occ
    return np.maximum(f32(1.0) - acc / f32(len(dirs)), f32(0.0)).astype(f32)


def fma_g(a):
    """sqrtf(fmaf(a, a, 1)) through binary64: a * a is exact there, and the sum rounds once more than fma does only in a double-
    rounding case that none of the ratios used here meets (asserted where it matters: the fields agree bit for bit)"""
    return f32(np.sqrt(f32(np.float64(a) * np.float64(a) + 1.0)))


@pytest.mark.parametrize("n,reach", [(33, 5.0), (130, 70.0)])
def test_the_model_agrees_with_a_numpy_restatement(n, reach):
    h = smooth(n, 4) + (np.random.default_rng(n).random((n, n), dtype=f32) * f32(0.02))
    h[3, 7] = np.nan
    h[n - 2, 5] = np.inf
    for dirs in (DIRS, DIRS[:1], abm.IRREGULAR):
        got = abm.field_heights(h, dirs, spacing=1.3, exag=0.8, reach=reach)
        want = brute_force(h, dirs, 1.3, 0.8, reach)
        assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())
        assert got[3, 7] == 1.0 and got[n - 2, 5] == 1.0 and ((got > 0.1) & (got < 0.9)).any()


def test_the_field_commutes_with_the_symmetries_of_the_grid():
    n = 97
    h = smooth(n, 3)
    off = np.array([d for d in DIRS if abs(d[0]) != abs(d[1])], f32)           # off the exact diagonal (a tie takes x in both problems)
    for d in off:
        d = d[None, :]
        f = abm.field_heights(h, d, exag=1.3, reach=20.0)
        assert np.array_equal(bits(abm.field_heights(h.T.copy(), d[:, ::-1], exag=1.3, reach=20.0)), bits(f.T)), d
        assert np.array_equal(bits(abm.field_heights(h[:, ::-1].copy(), d * f32([-1, 1]), exag=1.3, reach=20.0)), bits(f[:, ::-1])), d
        assert np.array_equal(bits(abm.field_heights(h[::-1, :].copy(), d * f32([1, -1]), exag=1.3, reach=20.0)), bits(f[::-1, :])), d
    # a whole set mirrored in the same order sums in the same order
    f = abm.field_heights(h, off, exag=1.3, reach=20.0)
    assert np.array_equal(bits(abm.field_heights(h[:, ::-1].copy(), off * f32([-1, 1]), exag=1.3, reach=20.0)), bits(f[:, ::-1]))
    assert (f < 1).any()


def test_the_field_does_not_know_strength_and_the_frame_does():
    import oracle
    W, H = 96, 64
    h = abm.scene_heights()
    lut = np.zeros(1024, np.uint8)
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["default"]), f32).reshape(44)
    rgba, vis = oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True, nthreads=8)
    sky = abm.field(u, h, GRID, abm.scene_directions(), 2.0)
    a, ma = abm.frame(rgba, vis, u, h, GRID, lut, sky, 0.8)
    b, mb = abm.frame(rgba, vis, u, h, GRID, lut, sky, 0.3)
    z, mz = abm.frame(rgba, vis, u, h, GRID, lut, sky, 0.0)
    assert np.array_equal(ma, mb) and ma.any() and not mz.any() and np.array_equal(z, rgba.reshape(H, W, 4))
    assert np.array_equal(a[~ma], rgba.reshape(H, W, 4)[~ma])


def test_sky_is_one_on_a_plane_and_down_a_tilted_one():
    n = 65
    for level in (0.0, 0.37, -2.0):
        assert (abm.field_heights(np.full((n, n), level, f32), DIRS, reach=30.0) == 1.0).all()
    x = np.arange(n, dtype=f32) * f32(0.125)                                  # (exact: every difference of two heights is)
    h = np.tile(x, (n, 1))                                                    # rises towards +x
    down = np.array([(-1, 0), (-0.9, 0.31), (-0.9, -0.31), (-1, 1)], f32)     # looking towards -x: nothing stands above the vertex
    assert (abm.field_heights(h, down, reach=30.0) == 1.0).all()
    up = abm.field_heights(h, np.array([(1, 0)], f32), reach=30.0)
    assert (up[:, :-1] < 1.0).all() and (up[:, -1] == 1.0).all()              # (the last column has no predecessor)


@pytest.mark.parametrize("d,m", [((1, 0), 1), ((1, 0), 5), ((0, -1), 3), ((1, 1), 2), ((-0.5, 1), 4)])
def test_a_single_step_gives_the_hand_computed_value(d, m):
    n, spacing, exag, Y = 65, 1.5, 0.5, 0.3
    ux, uz = d
    zmajor = abs(uz) > abs(ux)
    a = f32(min(abs(ux), abs(uz))) / f32(max(abs(ux), abs(uz)))
    # the vertex in the middle; the step m towards the direction: m along the major axis, rint(m a) across (from the middle the shear
    # of the line is what the contract's r(k) - r(k - m) gives when r(k) is itself whole: choose k accordingly)
    j0 = i0 = n // 2
    smaj, smin = (uz, ux) if zmajor else (ux, uz)
    k = n - 1 - (j0 if zmajor else i0) if smaj > 0 else (j0 if zmajor else i0)
    r = lambda q: int(np.rint(f32(q) * a))
    s = -1 if smin < 0 else 1
    dmaj = m if smaj > 0 else -m
    dmin = s * (r(k) - r(k - m))
    jj, ii = (j0 + dmaj, i0 + dmin) if zmajor else (j0 + dmin, i0 + dmaj)
    h = np.zeros((n, n), f32)
    h[jj, ii] = Y
    sky = abm.field_heights(h, np.array([d], f32), spacing=spacing, exag=exag, reach=40.0)
    g = fma_g(a)
    ell = ((f32(3.0) / (f32(n) - f32(1.0))) * f32(spacing)) * g
    T = (f32(Y) * f32(exag)) * (f32(1.0) / (f32(m) * ell))
    want = f32(1.0) - (f32(1.0) - f32(1.0) / (f32(1.0) + T * T))
    assert bits(sky[j0, i0]) == bits(want), (sky[j0, i0], want)
    assert abs(float(T) - Y * exag / (m * float(g) * 3.0 / (n - 1) * spacing)) < 1e-5 * float(T)


def test_the_reach_is_isotropic():
    """a spike is seen from exactly the vertices within `reach` cells of Euclidean distance along each direction's lines"""
    n, reach = 129, 20.0
    h = np.zeros((n, n), f32)
    c = n // 2
    h[c, c] = 1.0
    for d in DIRS:
        sky = abm.field_heights(h, d[None, :], reach=reach)
        seen = np.argwhere(sky < 1.0)
        assert len(seen)
        dist = np.hypot(seen[:, 0] - c, seen[:, 1] - c)
        a = min(abs(d[0]), abs(d[1])) / max(abs(d[0]), abs(d[1]))
        g = float(np.hypot(1.0, a))
        R = max(1, int(np.floor(reach / g)))
        # the farthest vertex that sees the spike is R steps away: R g cells along the ray, at most half a cell off it
        assert len(seen) == R, (d, len(seen), R)
        assert dist.max() <= reach + 0.5 and dist.max() > reach - g - 0.5, (d, dist.max())


@pytest.mark.parametrize("grid,exag,reach,D", abm.FIELD_CASES + abm.LIMIT_FIELD_CASES)
def test_the_gpu_tests_fields_are_partly_occluded(grid, exag, reach, D):
    import oracle
    limit = (grid, exag, reach, D) in abm.LIMIT_FIELD_CASES
    h = abm.limit_heights() if limit else heights(4, (97, 131))
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, 64, 64, *CAMERAS["default"]), f32).reshape(44)
    u[38] = exag
    sky = abm.field(u, h, grid, abm.case_directions(D), reach)
    assert ((sky > 0.1) & (sky < 0.9)).mean() > 0.1
    assert (sky >= 0).all() and (sky <= 1).all()
    if limit and reach == 1024.0:
        # the far half of the reach decides horizons: a scan that stops short differs.  Shown at a quarter of the grid and of the
        # reach: the bowl and the noise are stated in world units, so the same horizons lie a quarter as many steps away, and the
        # two fields cost a sixty-fourth of a second field at full size
        assert grid > reach
        g4, dirs = (grid + 3) // 4, abm.case_directions(D)
        assert g4 > reach / 4
        assert (abm.field(u, h, g4, dirs, reach / 4) != abm.field(u, h, g4, dirs, reach / 8)).mean() > 0.1


@pytest.mark.parametrize("size", [(96, 64), (256, 256)])
def test_the_gpu_tests_scene_is_partly_occluded(size):
    import oracle
    W, H = size
    h = abm.scene_heights()
    lut = np.load(os.path.join(HERE, "golden", "colormaps_rgba8.npz"))["viridis"]
    for cam in CAMERAS:
        u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam]), f32).reshape(44)
        u[32:35] = shm.sun_vector(*abm.SCENE_SUN_DEG)
        rgba, vis = oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True, nthreads=8)
        sky = abm.field(u, h, GRID, abm.scene_directions(), abm.SCENE_PARAMS["reach"])
        assert ((sky > 0.1) & (sky < 0.9)).mean() >= 0.1
        frame, again = abm.frame(rgba, vis, u, h, GRID, lut, sky, abm.SCENE_PARAMS["strength"])
        covered = int((vis != 0).sum())
        frac = again.sum() / covered
        assert covered > 0 and 0.1 <= frac <= 0.9, (cam, size, frac)
        assert not again[vis == 0].any()
        assert np.array_equal(frame[~again], rgba.reshape(H, W, 4)[~again])
        # with the cast shadows of the same scene no fewer pixels are written again, and some come out darker
        lit = shm.field(u, h, GRID, **abm.SCENE_SHADOWS)
        both, again2 = abm.frame(rgba, vis, u, h, GRID, lut, sky, abm.SCENE_PARAMS["strength"], lit=lit)
        assert (lit < 1).any() and (both != frame).any() and not (again & ~again2).any()
