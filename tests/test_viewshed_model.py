"""The viewshed CPU model (tests/viewshed_model) against what a viewshed must do: every vertex but the observer has
exactly one owning (line, step); a hand-worked wall hides what lies behind it by the worked amounts; flat ground is seen, a tall enough
target is seen, non-finite heights neither occlude nor hide; the field commutes with the eight symmetries of the square exactly; the
three-launch decomposition of the kernels, emulated in numpy, equals the sequential walk; a float64 restatement agrees; and the scene
the GPU tests draw is part hidden."""

import numpy as np
import pytest

from support import bits, smooth
import viewshed_model as vsm
from overlay_scenes import CAMERAS, GRID, heights


def r_of(L, c, k):
    """contract item 2 in Python integers"""
    return int(np.sign(c)) * ((2 * k * abs(c) + L) // (2 * L))


def owner_of(L, k, m):
    return int(np.sign(m)) * ((2 * abs(m) * L + k) // (2 * k))


# ---- item 2: ownership ----

def test_the_line_formulas_are_the_contracts_and_invert():
    lib = vsm.lib()
    for L in (1, 2, 3, 7, 12, 32, 202):
        ks = range(1, L + 1) if L <= 32 else (1, 2, 63, 64, 65, 101, L - 1, L)
        for k in ks:
            for m in range(-k, k + 1):
                c = owner_of(L, k, m)
                assert lib.vsm_owner(L, k, m) == c
                assert abs(c) <= L and r_of(L, c, k) == m and lib.vsm_minor(L, c, k) == m, (L, k, m, c)
    L = 8191                                                # grid 8192: the products stay inside 32 bits
    for k, m in ((8191, 8191), (8191, -8190), (1, 1), (4097, 4000)):
        c = owner_of(L, k, m)
        assert lib.vsm_owner(L, k, m) == c and lib.vsm_minor(L, c, k) == m
        assert 2 * k * abs(c) + L < 2 ** 32 and 2 * abs(m) * L + k < 2 ** 32


def observers(n):
    if n <= 12:
        return [(i, j) for j in range(n) for i in range(n)]
    m = n // 2
    return [(0, 0), (n - 1, 0), (0, n - 1), (n - 1, n - 1), (m, 0), (0, m), (n - 1, m), (m, n - 1), (m, m), (5, 11)]


@pytest.mark.parametrize("n", list(range(2, 13)) + [33])
def test_every_vertex_but_the_observer_has_one_owning_line_and_step(n):
    h = np.zeros((n, n), np.float32)
    for v in observers(n):
        seen, w = vsm.field_heights(h, v, writers=True)
        assert (w == 1).all(), (n, v, np.argwhere(w != 1)[:4].tolist())   # (the observer's own vertex is written once, apart from the lines)


# ---- item 3: the horizon ----

def test_a_hand_worked_wall():
    """5 x 5, L = 4, the observer at vertex (0, 2) with its eye 1 above flat ground at 0; column i = 2 is a wall of height 2.
    softness 4, bias 0, so seen = 1 - e / 4 where 0 <= e <= 4.  Row j = 2 is line c = 0 of the +x quadrant, D = k:
        k = 1: y = 0, first step: seen 1;                                             t = (0 - 1) / 1 = -1
        k = 2: the wall: s = (2 - 1) / 2 = 0.5, e = (-1 - 0.5) 2 = -3 < 0: seen 1;      t = 0.5
        k = 3: s = (0 - 1) / 3, e = (0.5 + 1/3) 3 = 2.5: seen 1 - 2.5 / 4 = 0.375
        k = 4: s = -0.25, e = (0.5 + 0.25) 4 = 3: seen 0.25
    Vertex (4, 4): offset (4, 2), x-major, c* = floor((2 2 4 + 4) / 8) = 2; line 2 holds r = floor((4 k + 4) / 8) = 1, 1, 2, 2 at
    k = 1 ... 4, so it passes the wall at (2, 3): D = sqrt(5), t = 1 / sqrt(5); the target: D = sqrt(20), s = -1 / sqrt(20),
    e = (1 / sqrt(5) + 1 / sqrt(20)) sqrt(20) = 2 + 1 = 3: seen 0.25.  The columns i = 0, 1 and the wall itself are seen."""
    h = np.zeros((5, 5), np.float32)
    h[:, 2] = 2.0
    seen = vsm.field_heights(h, (0, 2), eye_height=1.0, softness=4.0, bias=0.0)
    assert (seen[:, :3] == 1.0).all()
    assert seen[2, 4] == 0.25
    assert abs(seen[2, 3] - 0.375) <= 2e-7                  # (1 / 3 is rounded)
    assert abs(seen[4, 4] - 0.25) <= 2e-7 and abs(seen[0, 4] - 0.25) <= 2e-7
    assert (seen[:, 3:] < 1.0).all() and (seen[:, 3:] >= 0.0).all()
    # a sharp edge: the same scene is 0 / 1
    sharp = vsm.field_heights(h, (0, 2), eye_height=1.0, softness=1e-6, bias=0.0)
    assert (sharp[:, :3] == 1.0).all() and (sharp[:, 3:] == 0.0).all()
    # eye above the wall's top by enough: everything is seen again
    assert (vsm.field_heights(h, (0, 2), eye_height=10.0, softness=1e-6, bias=0.0) == 1.0).all()


def test_flat_ground_is_seen_from_above_it():
    for n, level in ((65, 0.0), (33, 0.37), (130, -2.0)):
        h = np.full((n, n), level, np.float32)
        for v in observers(33)[:9] + [(n - 1, n // 3)]:
            assert (vsm.field_heights(h, v, eye_height=0.05) == 1.0).all(), (n, level, v)


def test_a_tall_enough_target_is_seen():
    h = smooth(65, 4) * np.float32(2.0)
    low = vsm.field_heights(h, (10, 50), eye_height=0.01)
    assert (low < 1.0).mean() > 0.2
    span = float(h.max() - h.min())
    # the horizon's slope is at most span / 1 (per cell), the target 64 sqrt(2) cells away at most: 200 spans lift it over any horizon
    assert (vsm.field_heights(h, (10, 50), eye_height=0.01, target_height=200.0 * span) == 1.0).all()


def test_non_finite_heights_neither_occlude_nor_hide():
    h = smooth(65, 2)
    for v in ((0, 0), (32, 32), (64, 10), (7, 40)):
        for bad in (np.nan, np.inf, -np.inf):
            g, low = h.copy(), h.copy()
            g[20, 30] = g[40, 41] = bad
            low[20, 30] = low[40, 41] = -1e30                # a pit occludes nothing either
            f, want = vsm.field_heights(g, v), vsm.field_heights(low, v)
            assert f[20, 30] == 1.0 and f[40, 41] == 1.0
            want[20, 30] = want[40, 41] = 1.0
            assert np.array_equal(bits(f), bits(want)), (v, bad)
    g = h.copy()
    g[32, 32] = np.nan                                       # an observer without a height: the whole field is 1
    assert (vsm.field_heights(g, (32, 32)) == 1.0).all()
    assert (vsm.field_heights(np.full((33, 33), np.nan, np.float32), (3, 4)) == 1.0).all()
    assert (vsm.field_heights(h, (7, 40)) < 1.0).any()


def test_the_field_commutes_with_the_eight_symmetries_of_the_square():
    n, P = 97, dict(exag=1.3, eye_height=0.03, target_height=0.01, softness=0.05, bias=0.002)
    h = smooth(n, 3)
    for io, jo in ((0, 0), (96, 40), (48, 48), (13, 77), (50, 0)):
        f = vsm.field_heights(h, (io, jo), **P)
        assert (f < 1.0).any() and (f == 1.0).any()
        for transpose in (False, True):
            for mi in (False, True):
                for mj in (False, True):
                    g, v = h, (io, jo)
                    want = f
                    if transpose:
                        g, v, want = g.T, (v[1], v[0]), want.T
                    if mi:
                        g, v, want = g[:, ::-1], (n - 1 - v[0], v[1]), want[:, ::-1]
                    if mj:
                        g, v, want = g[::-1, :], (v[0], n - 1 - v[1]), want[::-1, :]
                    got = vsm.field_heights(np.ascontiguousarray(g), v, **P)
                    assert np.array_equal(bits(got), bits(want)), ((io, jo), transpose, mi, mj)


# ---- the kernels' decomposition, and a float64 restatement ----

def numpy_field(h, vertex, exag, eye_height, target_height, softness, bias, dtype, chunk=None):
    """Items 1-3 restated on whole (line, step) arrays in `dtype`.  chunk: None -- a running maximum along every line; 64 -- the
    three launches of vf_viewshed.h: the maximum of every chunk of every line, their exclusive running maximum along the line, the
    inclusive scan inside a chunk shifted by one step and joined with the carry."""
    T = dtype
    n = h.shape[0]
    L = n - 1
    io, jo = vertex
    y_all = (h.astype(T) * T(exag))
    seen = np.ones((n, n), T)
    y_obs = y_all[jo, io]
    if not np.isfinite(y_obs):
        return seen
    y_eye = y_obs + T(eye_height)
    for q, steps in enumerate((n - 1 - io, io, n - 1 - jo, jo)):
        if steps == 0:
            continue
        zmajor, sign = q >= 2, -1 if q & 1 else 1
        c = np.arange(-L, L + 1, dtype=np.int64)[:, None]
        k = np.arange(1, steps + 1, dtype=np.int64)[None, :]
        r = np.sign(c) * ((2 * k * np.abs(c) + L) // (2 * L))
        minor = (io if zmajor else jo) + r
        major = (jo if zmajor else io) + sign * k + 0 * c
        exists = (minor >= 0) & (minor < n)
        mi = np.clip(minor, 0, n - 1)
        jj, ii = (major, mi) if zmajor else (mi, major)
        y = np.where(exists, y_all[jj, ii], T(np.nan))
        D = np.sqrt((k * k + r * r).astype(T))
        fin = np.isfinite(y)
        with np.errstate(invalid="ignore"):
            t = np.where(fin, (y - y_eye) / D, T(-np.inf)).astype(T)
        if chunk is None:
            inc = np.maximum.accumulate(t, axis=1)
            M = np.concatenate([np.full((t.shape[0], 1), -np.inf, T), inc[:, :-1]], axis=1)
        else:
            nch = (steps + chunk - 1) // chunk
            pad = np.full((t.shape[0], nch * chunk - steps), -np.inf, T)
            tc = np.concatenate([t, pad], axis=1).reshape(t.shape[0], nch, chunk)
            cmax = tc.max(axis=2)                                                         # launch 1
            run = np.maximum.accumulate(cmax, axis=1)
            carry = np.concatenate([np.full((t.shape[0], 1), -np.inf, T), run[:, :-1]], axis=1)   # launch 2
            inc = np.maximum.accumulate(tc, axis=2)                                       # launch 3: the wave's scan ...
            before = np.concatenate([np.full(inc.shape[:2] + (1,), -np.inf, T), inc[:, :, :-1]], axis=2)
            M = np.maximum(before, carry[:, :, None]).reshape(t.shape[0], nch * chunk)[:, :steps]
        with np.errstate(invalid="ignore", over="ignore"):
            s = ((y + T(target_height)) - y_eye) / D
            e = (M - s) * D
            val = T(1) - np.minimum(np.maximum((e - T(bias)) / T(softness), T(0)), T(1))
        cstar = np.sign(r) * ((2 * np.abs(r) * L + k) // (2 * k))
        owned = exists & (cstar == c) & ((np.abs(r) < k) if zmajor else True)
        put = owned & fin
        seen[jj[put], ii[put]] = val[put].astype(T)
    return seen


@pytest.mark.parametrize("n", [130, 203, 66])
def test_the_three_launch_decomposition_equals_the_sequential_walk(n):
    P = dict(exag=0.8, eye_height=0.04, target_height=0.0, softness=0.05, bias=0.003)
    h = smooth(n, 6)
    h[n // 3, n // 2] = np.nan
    for v in ((0, 0), (n - 1, n // 2), (n // 2, n // 2), (n - 3, 41), (1, n - 1)):
        want = vsm.field_heights(h, v, **P)
        got = numpy_field(h, v, dtype=np.float32, chunk=64, **P)
        assert np.array_equal(bits(got), bits(want)), (n, v, int((bits(got) != bits(want)).sum()))
        assert (want < 1).any()


def test_a_float64_restatement_agrees():
    """softness 0.1 on a smooth surface: seen moves by the error of e over the softness.  The binary32 error of e is of the order of
    1e-5 here (a slope to 2^-24 relative, times a distance below 46 cells, times heights below 1): 1e-3 leaves room."""
    n, P = 33, dict(exag=1.2, eye_height=0.05, target_height=0.0, softness=0.1, bias=0.002)
    h = smooth(n, 11)
    worst = 0.0
    for v in ((0, 0), (32, 16), (16, 16), (5, 27), (32, 32)):
        got = vsm.field_heights(h, v, **P)
        want = numpy_field(h, v, dtype=np.float64, **P)
        worst = max(worst, float(np.abs(got - want).max()))
        assert (want < 1).any() and (want > 0).any()
    print(f"binary32 model against float64: max |d seen| = {worst:.3g}")
    assert worst <= 1e-3


# ---- item 1 and the frame ----

def test_the_observer_snaps_to_the_nearest_vertex_and_is_clamped():
    n = 129
    step = 3.0 / (n - 1)
    assert vsm.observer_vertex((0.0, 0.0), 1.0, n) == (64, 64)
    assert vsm.observer_vertex((-1.5, 1.5), 1.0, n) == (0, n - 1)
    assert vsm.observer_vertex((-9.0, 40.0), 1.0, n) == (0, n - 1)            # outside the grid: clamped
    assert vsm.observer_vertex((-1.5 + 10.4 * step, -1.5 + 10.6 * step), 1.0, n) == (10, 11)
    assert vsm.observer_vertex((2.0 * (-1.5 + 10.4 * step), 2.0 * (-1.5 + 10.6 * step)), 2.0, n) == (10, 11)   # the overlays' frame: times spacing


@pytest.mark.parametrize("size", [(640, 360), (257, 131)])
def test_the_gpu_tests_scene_is_part_hidden(size):
    import oracle
    W, H = size
    h = heights()
    lut = np.zeros(1024, np.uint8)
    for cam in CAMERAS:
        u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam]), np.float32).reshape(44)
        rgba, vis = oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True, nthreads=8)
        seen, v = vsm.field(u, h, GRID, vsm.SCENE_OBSERVER, **vsm.SCENE_PARAMS)
        frame, s = vsm.frame(rgba, vis, u, h, GRID, seen, v, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))
        covered = vis != 0
        frac = float((s[covered] < 0.5).mean())
        assert covered.any() and 0.1 <= frac <= 0.9, (cam, size, frac)
        assert (s[~covered] == -1.0).all() and (s[covered] >= 0.0).all() and (s[covered] <= 1.0).all()
        assert np.array_equal(frame[~covered], rgba.reshape(H, W, 4)[~covered])           # background pixels are never touched
        assert (frame[covered] != rgba.reshape(H, W, 4)[covered]).any()
        # colours with alpha 0 write nothing; a radius treats only pixels near the observer
        none, _ = vsm.frame(rgba, vis, u, h, GRID, seen, v, visible_rgba=(64, 255, 96, 0), hidden_rgba=(0, 0, 0, 0))
        assert np.array_equal(none, rgba.reshape(H, W, 4))
        near, sr = vsm.frame(rgba, vis, u, h, GRID, seen, v, radius=0.6, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))
        inside = sr >= 0.0
        assert not inside[~covered].any() and np.array_equal(near[inside], frame[inside])
        assert np.array_equal(near[~inside], rgba.reshape(H, W, 4)[~inside])
        if cam != "near":
            assert inside.any() and (covered & ~inside).any(), cam
