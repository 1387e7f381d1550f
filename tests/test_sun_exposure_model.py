"""Sun exposure's CPU model (tests/sun_exposure_model) against what a sum of shadow fields must do: one sun of weight 1
gives the quantised shadow field; the order of the suns changes no bit; flat ground gets every counted sun in full; suns on or below
the horizon and suns of weight 0 add nothing; a hand-worked wall with a sun on either side gives the worked sums; the incidence
cosine of a tilted plane is the analytic one; halving the weights never raises a sum; and the scene the GPU tests compute is not a
trivial one."""

import numpy as np
import pytest

from support import smooth
import shadow_model as shm
import sun_exposure_model as sem
from overlay_scenes import heights

F32 = np.float32


def scene_uniforms(exag=0.6, spacing=1.0):
    u = np.zeros(44, np.float32)
    u[36], u[38] = spacing, exag
    return u


def test_the_scene_suns_are_what_the_design_says():
    assert sem.SUNS.shape == (34, 3) and sem.SUNS.dtype == np.float32 and sem.WEIGHTS.shape == (34,)
    arc = sem.ARC
    assert int((arc[:, 1] <= 0).sum()) == 2 and arc[0, 1] < 0 and arc[-1, 1] < 0
    zmajor = np.abs(arc[:, 2]) > np.abs(arc[:, 0])
    assert int(zmajor.sum()) == 12 and int((~zmajor).sum()) == 12
    assert sem.WEIGHTS[3] == 0.0 and sem.WEIGHTS[5] == 1.0 and ((sem.WEIGHTS >= 0) & (sem.WEIGHTS <= 1)).all()
    assert ((sem.ARC_WEIGHTS > 0) & (sem.ARC_WEIGHTS < 1)).all()
    assert int(sem.counted(sem.SUNS).sum()) == 30                 # two of the arc and two of the vectors are not counted
    assert np.array_equal(sem.SUNS[24], (0, 1, 0)) and np.array_equal(sem.SUNS[32], (F32(0.3), 0, 1)) and sem.SUNS[33, 1] < 0


def test_one_sun_of_weight_one_gives_the_quantised_shadow_field():
    h = smooth(65, 3) * F32(2.0)
    for sun in ((0.9, 0.3, 0.31), (-0.31, 0.2, 0.9), (1.0, 0.4, 0.0), (0.5, 0.3, -0.5), (0.0, 1.0, 0.0)):
        lit = shm.field_heights(h, sun, 1.0, 1.0, 1.0, 0.02, 0.002)
        total = sem.sum_heights(h, [sun])
        want = np.rint(lit.astype(np.float64) * 65536.0) / 65536.0        # (exact in float64, and in float32: q <= 65536 has 17 bits)
        assert np.array_equal(sem.exposure(total).astype(np.float64), want)
        assert total.max() == 65536 and np.abs(sem.exposure(total) - lit).max() <= 2.0 ** -17
        if sun[0] or sun[2]:
            assert (total < 65536).any()


def test_the_order_of_the_suns_changes_no_bit():
    h = smooth(65, 5) * F32(2.0)
    for incidence in (False, True):
        want = sem.sum_heights(h, sem.SUNS, sem.WEIGHTS, incidence=incidence)
        for seed in range(3):
            order = np.random.default_rng(seed).permutation(len(sem.SUNS))
            assert np.array_equal(sem.sum_heights(h, sem.SUNS[order], sem.WEIGHTS[order], incidence=incidence), want)
        twice = sem.sum_heights(h, np.concatenate([sem.SUNS, sem.SUNS[6:7]]), np.concatenate([sem.WEIGHTS, sem.WEIGHTS[6:7]]), incidence=incidence)
        assert np.array_equal(twice - want, sem.sum_heights(h, sem.SUNS[6:7], sem.WEIGHTS[6:7], incidence=incidence))   # (the same sun twice counts twice)


def test_flat_ground_gets_every_counted_sun_in_full():
    for n, level in ((33, 0.25), (65, -2.0)):
        h = np.full((n, n), level, np.float32)
        on = sem.counted(sem.SUNS)
        total = sem.sum_heights(h, sem.SUNS, sem.WEIGHTS)
        want = sum(int(np.rint(np.float64(w) * 65536.0)) for w in sem.WEIGHTS[on])
        assert (total == want).all()
        wtot = sem.weight_total(sem.SUNS, sem.WEIGHTS)
        assert abs(float(sem.exposure(total)[0, 0]) - float(wtot)) <= 30 * 2.0 ** -17 + 30 * 2.0 ** -22
        assert (sem.sum_heights(h, sem.SUNS) == 30 * 65536).all() and (sem.fraction(sem.exposure(sem.sum_heights(h, sem.SUNS)), 30.0) == 1.0).all()
        # with incidence: the normal is straight up, c = sy / |s| in binary32, clamped, then times the weight, then quantised -- per sun
        want = 0
        for s, w in zip(sem.SUNS[on], sem.WEIGHTS[on]):
            sl = np.sqrt(F32(F32(s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
            c = min(F32(s[1] / sl), F32(1.0))
            want += int(np.rint(F32(F32(c * w) * F32(65536.0))))
        assert (sem.sum_heights(h, sem.SUNS, sem.WEIGHTS, incidence=True) == want).all()


def test_suns_on_or_below_the_horizon_and_weights_of_zero_add_nothing():
    h = smooth(65, 2) * F32(2.0)
    up = np.array([(0.9, 0.3, 0.31), (-0.2, 0.5, 0.7)], F32)
    down = np.array([(0.3, 0.0, 1.0), (0.5, -0.2, 0.1), (0.0, 0.0, 0.0), (0.0, -1.0, 0.0), (1.0, -0.0, 0.0)], F32)
    for incidence in (False, True):
        base = sem.sum_heights(h, up, incidence=incidence)
        assert np.array_equal(sem.sum_heights(h, np.concatenate([down[:2], up, down[2:]]), incidence=incidence), base)
        assert (sem.sum_heights(h, down, incidence=incidence) == 0).all()
        w0 = sem.sum_heights(h, np.concatenate([up, up]), np.array([1, 1, 0, 0], F32), incidence=incidence)
        assert np.array_equal(w0, base)
    assert sem.weight_total(down) == 0.0 and (sem.fraction(sem.exposure(sem.sum_heights(h, down)), 0.0) == 0.0).all()
    assert not sem.counted(down).any() and sem.counted(up).all()
    assert sem.weight_total(np.concatenate([up, down]), np.array([0.5, 0.25, 1, 1, 1, 1, 1], F32)) == 0.75


def test_a_hand_worked_wall_with_a_sun_on_either_side():
    """5 x 5 vertices at spacing 4: step = 3 / 4, a cell is 3 wide.  Column i = 2 is a wall of height 6 on flat ground; softness 4,
    bias 0.  Sun A = (1, 1, 0) stands in +x at 45 degrees: the ray rises d = 3 per step, steps count from i = 4.  At i = 1 (step 3)
    the wall's term is 6 + 2 * 3 = 12, the ray is at 12 - 3 * 3 = 3 above the ground: e = 3, lit = 1 - 3 / 4 = 0.25; at i = 0 it is
    at 12 - 12 = 0: lit.  Sun B = (-1, 1, 0) is the mirror image.  So both suns give 131072 everywhere but 65536 + 16384 in the
    columns 1 and 3.  With weights 0.5 (A) and 1 (B): column 1 has 0.25 * 0.5 + 1, column 3 has 0.5 + 0.25.
    With incidence the flat columns 0, 4 and the wall's top (central difference 0) have c = 1 / sqrt(2) for both suns, q = 46341 each;
    in column 1 the slope is px = (6 - 0) / 6 = 1: A grazes it (c = 0), B meets it head on (c = 1, lit = 1)."""
    h = np.zeros((5, 5), np.float32)
    h[:, 2] = 6.0
    A, B = (1.0, 1.0, 0.0), (-1.0, 1.0, 0.0)
    kw = dict(spacing=4.0, softness=4.0, bias=0.0)
    total = sem.sum_heights(h, [A, B], **kw)
    assert (total[:, [0, 2, 4]] == 131072).all() and (total[:, [1, 3]] == 65536 + 16384).all()
    only_a = sem.sum_heights(h, [A], **kw)
    assert (only_a[:, 1] == 16384).all() and (np.delete(only_a, 1, axis=1) == 65536).all()
    weighted = sem.sum_heights(h, [A, B], [0.5, 1.0], **kw)
    assert (weighted[:, 1] == 8192 + 65536).all() and (weighted[:, 3] == 32768 + 16384).all() and (weighted[:, [0, 2, 4]] == 98304).all()
    e = sem.exposure(weighted)
    assert e[0, 1] == 1.125 and e[0, 3] == 0.75 and e[0, 0] == 1.5
    assert sem.weight_total([A, B], [0.5, 1.0]) == 1.5 and sem.fraction(e, 1.5)[0, 0] == 1.0 and sem.fraction(e, 1.5)[0, 3] == 0.5
    inc = sem.sum_heights(h, [A, B], incidence=True, **kw)
    assert (inc[:, [0, 2, 4]] == 2 * 46341).all()
    assert (inc[:, 1] == 65536).all() and (inc[:, 3] == 65536).all()
    assert np.array_equal(inc, inc[:, ::-1]) and np.array_equal(total, total[:, ::-1])


def ulps(a, b):
    """the distance of two positive float32 arrays in units in the last place"""
    return np.abs(np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64) - np.ascontiguousarray(b, F32).view(np.int32).astype(np.int64))


def test_the_cosine_of_a_tilted_plane_is_the_analytic_one():
    """n = 49 at spacing 1: a cell is 1 / 16 exactly, and the plane y = (a i + b j) / 16 with a = 0.5, b = -0.25 has exact heights and
    exact differences, so px = a and pz = b without an error.  The suns have integer components and an integer length, so the
    numerator and the sun's length are exact too: what is left is the rounding of sqrt(1 + a a + b b), and of the two divisions, half
    an ulp each."""
    n, a, b = 49, 0.5, -0.25
    jj, ii = np.mgrid[0:n, 0:n]
    h = ((a * ii + b * jj) / 16.0).astype(F32)
    for sun in ((3, 12, 4), (-4, 12, 3), (2, 6, -3), (12, 4, 3), (0, 1, 0), (-12, 3, -4)):
        want = (sun[1] - a * sun[0] - b * sun[2]) / np.sqrt(1.0 + a * a + b * b) / np.sqrt(float(sum(c * c for c in sun)))
        c = sem.cosine(h, sun)
        if want <= 0:
            assert (c == 0).all(), sun
            continue
        assert 0 < want < 1
        inside = c[1:-1, 1:-1]
        assert ulps(inside, np.full_like(inside, F32(want))).max() <= 2, sun
        assert (inside == inside[0, 0]).all()
        assert ulps(c, np.full_like(c, F32(want))).max() <= 2          # (a plane: the one-sided differences of the edges are exact as well)
    # exaggeration and spacing scale the slopes: twice the spacing at twice the exaggeration is the same surface
    assert np.array_equal(sem.cosine(h, (3, 12, 4), spacing=2.0, exag=2.0), sem.cosine(h, (3, 12, 4)))
    # a hole: 0 on the vertex and on its four neighbours, whose differences read it; the diagonal neighbours do not
    g = h.copy()
    g[20, 30] = np.nan
    c = sem.cosine(g, (3, 12, 4))
    for j, i in ((20, 30), (19, 30), (21, 30), (20, 29), (20, 31)):
        assert c[j, i] == 0.0
    rest = np.ones((n, n), bool)
    rest[[20, 19, 21, 20, 20], [30, 30, 30, 29, 31]] = False
    assert np.array_equal(c[rest], sem.cosine(h, (3, 12, 4))[rest]) and (c[rest] > 0).all()
    g[20, 30] = np.inf
    assert sem.cosine(g, (3, 12, 4))[20, 30] == 0.0 and sem.cosine(g, (3, 12, 4))[20, 31] == 0.0
    total = sem.sum_heights(g, [(3, 12, 4)], incidence=True)
    assert total[20, 30] == 0 and total[20, 29] == 0 and total[19, 29] > 0


def test_halving_every_weight_never_raises_a_sum():
    h = smooth(65, 7) * F32(2.0)
    for incidence in (False, True):
        full = sem.sum_heights(h, sem.SUNS, sem.WEIGHTS, incidence=incidence)
        half = sem.sum_heights(h, sem.SUNS, sem.WEIGHTS * F32(0.5), incidence=incidence)
        assert (half <= full).all() and (half < full).any()
        # (halving is exact, so a sun's q halves up to its rounding: half a step per counted sun)
        assert np.abs(2.0 * half.astype(np.float64) - full.astype(np.float64)).max() <= 30


@pytest.mark.parametrize("grid", [130, 203])
def test_the_gpu_tests_scene_is_not_trivial(grid):
    """heights(4, (97, 131)) at exaggeration 0.6, spacing 1, default softness and bias, under the 34 suns: much of the ground gets
    little sun, much of it more than half, and with the arc alone many sums are 0 and most of the rest fractional."""
    h = heights(4, (97, 131))
    u = scene_uniforms()
    nv = grid * grid
    wtot = sem.weight_total(sem.SUNS, sem.WEIGHTS)
    f = sem.fraction(sem.field(u, h, grid, sem.SUNS, sem.WEIGHTS), wtot)
    low, high = int((f < 0.1).sum()), int((f >= 0.5).sum())
    print(f"grid {grid}: {100 * low / nv:.1f} % below 0.1, {100 * high / nv:.1f} % at 0.5 and more")
    assert low >= 0.30 * nv and high >= 0.25 * nv
    assert f.max() <= 1.0 and f.min() >= 0.0
    fi = sem.fraction(sem.field(u, h, grid, sem.SUNS, sem.WEIGHTS, incidence=True), wtot)
    low, high = int((fi < 0.1).sum()), int((fi >= 0.5).sum())
    print(f"grid {grid}, incidence: {100 * low / nv:.1f} % below 0.1, {100 * high / nv:.1f} % at 0.5 and more, max {fi.max():.3f}")
    assert low >= 0.50 * nv and high >= 0.01 * nv and fi.max() >= 0.6
    assert (fi <= f).all()
    total = sem.field(u, h, grid, sem.ARC, sem.ARC_WEIGHTS, want_sum=True)[1]
    zero, frac = int((total == 0).sum()), int((total % 65536 != 0).sum())
    print(f"grid {grid}, the arc alone: {100 * zero / nv:.1f} % at 0, {100 * frac / nv:.1f} % fractional")
    assert zero >= 0.20 * nv and frac >= 0.40 * nv
