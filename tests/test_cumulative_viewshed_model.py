"""The cumulative viewshed's CPU model (tests/cumulative_viewshed_model) against what a cumulative viewshed must do:
one observer gives the quantised single field; the order of the observers changes no bit; flat ground seen from above counts N
everywhere; the hand-worked wall of the viewshed model with an observer on either side gives the worked sums; a larger radius never
lowers a count and the radius mask is a disc of grid vertices; a blind observer adds 1 everywhere in range; and the scene the GPU tests
compute is not a trivial one."""

import numpy as np
import pytest

from support import smooth
import cumulative_viewshed_model as cvm
import viewshed_model as vsm
from overlay_scenes import heights
from test_gpu_viewshed import PARAMS


def scene_uniforms(exag=0.6, spacing=1.0):
    u = np.zeros(44, np.float32)
    u[36], u[38] = spacing, exag
    return u


def test_one_observer_gives_the_quantised_single_field():
    h = smooth(65, 3) * np.float32(2.0)
    for v in ((0, 0), (32, 32), (64, 10), (7, 40)):
        seen = vsm.field_heights(h, v, **PARAMS)
        total = cvm.sum_heights(h, [v], **PARAMS)
        want = np.rint(seen.astype(np.float64) * 65536.0) / 65536.0       # (exact in float64, and in float32: q <= 65536 has 17 bits)
        assert np.array_equal(cvm.count(total).astype(np.float64), want)
        assert total.max() == 65536 and total[v[1], v[0]] == 65536 and (total < 65536).any()
        assert np.abs(cvm.count(total) - seen).max() <= 2.0 ** -17


def test_the_order_of_the_observers_changes_no_bit():
    h = smooth(65, 5) * np.float32(2.0)
    rng = np.random.default_rng(11)
    vertices = [tuple(int(c) for c in v) for v in rng.integers(0, 65, (12, 2))] + [(3, 3), (3, 3)]    # (two on one vertex both count)
    want = cvm.sum_heights(h, vertices, rc_cells=np.float32(30.5), **PARAMS)
    for seed in range(3):
        order = np.random.default_rng(seed).permutation(len(vertices))
        assert np.array_equal(cvm.sum_heights(h, [vertices[k] for k in order], rc_cells=np.float32(30.5), **PARAMS), want)
    once = cvm.sum_heights(h, vertices[:-1], rc_cells=np.float32(30.5), **PARAMS)
    assert np.array_equal(want - once, cvm.sum_heights(h, [(3, 3)], rc_cells=np.float32(30.5), **PARAMS))


def test_flat_ground_from_above_counts_every_observer_everywhere():
    for n, N in ((33, 1), (65, 7), (130, 40)):
        h = np.full((n, n), 0.25, np.float32)
        rng = np.random.default_rng(n)
        vertices = [tuple(int(c) for c in v) for v in rng.integers(0, n, (N, 2))]
        c = cvm.count(cvm.sum_heights(h, vertices, eye_height=0.05))
        assert (c == np.float32(N)).all()
        assert (cvm.fraction(c, N) == 1.0).all()


def test_a_hand_worked_wall_with_an_observer_on_either_side():
    """The wall of tests/test_viewshed_model.py (5 x 5, column i = 2 of height 2 on flat ground, eye 1 above it, softness 4, bias 0)
    with observer A at vertex (0, 2) and its mirror image B at (4, 2).  A sees columns 0 ... 2 and, behind the wall, (3, 2) by
    0.375, (4, 2) by 0.25 and the corners (4, 0) and (4, 4) by 0.25; B the mirror image.  So the wall counts 2 = 131072 / 65536;
    B's own vertex (4, 2) counts 1 + 0.25, q = 65536 + 16384 = 81920; the corners 1.25 up to the rounding of 1 / sqrt(5), which
    the quantisation (half a step of 2^-16) swallows or passes on as one step; (3, 2) counts 1 + rint(0.375 * 65536 +- 0.02) / 65536
    = 1 + 24576 / 65536."""
    h = np.zeros((5, 5), np.float32)
    h[:, 2] = 2.0
    kw = dict(eye_height=1.0, softness=4.0, bias=0.0)
    total = cvm.sum_heights(h, [(0, 2), (4, 2)], **kw)
    assert (total[:, 2] == 131072).all()
    assert total[2, 4] == 81920 and total[2, 0] == 81920
    assert total[2, 3] == 65536 + 24576 and total[2, 1] == 65536 + 24576
    for j, i in ((0, 0), (0, 4), (4, 0), (4, 4)):
        assert abs(int(total[j, i]) - 81920) <= 1
    assert np.array_equal(total, total[:, ::-1]) and np.array_equal(total, total[::-1, :])
    c = cvm.count(total)
    assert c[2, 4] == 1.25 and c[0, 2] == 2.0 and c[2, 3] == 1.375
    assert (total >= 65536).all()                              # (every vertex is in front of the wall for one of the two)
    sharp = cvm.sum_heights(h, [(0, 2), (4, 2)], eye_height=1.0, softness=1e-6, bias=0.0)
    assert (sharp[:, 2] == 131072).all() and (np.delete(sharp, 2, axis=1) == 65536).all()


def test_a_larger_radius_never_lowers_a_count_and_the_mask_is_a_disc():
    h = smooth(65, 7) * np.float32(2.0)
    vertices = [(0, 0), (32, 32), (64, 10), (7, 40), (40, 7)]
    full = cvm.sum_heights(h, vertices, **PARAMS)
    last = None
    for r in (0.3, 1.0, 2.5, 10.0, 31.99, 64.0, 90.6, 1e9, np.inf):
        total = cvm.sum_heights(h, vertices, rc_cells=np.float32(r), **PARAMS)
        assert (total <= full).all()
        if last is not None:
            assert (total >= last).all() and (r > 64.0 or (total > last).any())
        last = total
        for v in vertices:
            assert total[v[1], v[0]] >= 65536                  # (the observer's own vertex always counts)
    assert np.array_equal(last, full)
    assert np.array_equal(cvm.sum_heights(h, vertices, rc_cells=np.float32(90.6), **PARAMS), full)    # 64 sqrt(2) = 90.51
    m = cvm.in_range(65, (32, 32), np.float32(10.0))
    jj, ii = np.mgrid[0:65, 0:65]
    assert np.array_equal(m, (ii - 32) ** 2 + (jj - 32) ** 2 <= 100) and m[32, 42] and not m[33, 42]
    # a vertex inside the radius of one observer keeps that observer's bits: the cut changes which vertices count, not their values
    one = cvm.sum_heights(h, [(32, 32)], **PARAMS)
    cut = cvm.sum_heights(h, [(32, 32)], rc_cells=np.float32(10.0), **PARAMS)
    assert np.array_equal(cut[m], one[m]) and (cut[~m] == 0).all()
    # the radius in cells is formed in binary32 from the world radius, the spacing and the step
    assert cvm.rc(1.1, 1.0, 130) == np.float32(1.1) / (np.float32(1.0) * (np.float32(3.0) / np.float32(129.0)))
    assert [int(np.ceil(cvm.rc(1.1, 1.0, n))) for n in (130, 203, 257)] == [48, 75, 94]
    assert [int(cvm.rc(1.1, 1.0, n)) for n in (130, 203, 257)] == [47, 74, 93]


def test_a_blind_observer_adds_one_everywhere_in_range():
    h = smooth(65, 2) * np.float32(2.0)
    g = h.copy()
    g[30, 20] = np.nan                                         # the observer (20, 30) stands on a hole
    others = [(5, 5), (60, 33)]
    base = cvm.sum_heights(g, others, **PARAMS)
    assert np.array_equal(cvm.sum_heights(g, others + [(20, 30)], **PARAMS) - base, np.full((65, 65), 65536, np.uint32))
    m = cvm.in_range(65, (20, 30), np.float32(12.5))
    got = cvm.sum_heights(g, others + [(20, 30)], rc_cells=np.float32(12.5), **PARAMS)
    alone = cvm.sum_heights(g, others, rc_cells=np.float32(12.5), **PARAMS)
    assert np.array_equal(got - alone, np.where(m, 65536, 0).astype(np.uint32)) and 0 < m.sum() < 65 * 65
    # a hole that is not under an observer is seen by everybody whose range it lies in, and hides nothing
    assert base[30, 20] == 2 * 65536


@pytest.mark.parametrize("grid", [130, 203])
def test_the_gpu_tests_scene_is_not_trivial(grid):
    """heights(4, (97, 131)) at exaggeration 0.6 with the 70 observers: part of the ground is seen by nobody, most of it by some and
    partly, and some of it by all."""
    observers = cvm.scene_observers()
    N = len(observers)
    assert N == 70
    h = heights(4, (97, 131))
    cnt, vertices, total = cvm.field(scene_uniforms(), h, grid, observers, want_sum=True, **PARAMS)
    nv = grid * grid
    zero, frac, full = int((total == 0).sum()), int((total % 65536 != 0).sum()), int((total == N * 65536).sum())
    print(f"grid {grid}: {100 * zero / nv:.2f} % at 0, {100 * frac / nv:.2f} % fractional, {100 * full / nv:.3f} % at N")
    assert zero >= 0.05 * nv and frac >= 0.25 * nv and full > 0
    assert cnt.max() == N and cnt.min() == 0.0
    assert len(set(vertices)) >= 60
    # the radii of the GPU tests: one chunk, across the boundary at step 64, two chunks; and a small one
    for radius in (1.1, 0.25):
        part = cvm.field(scene_uniforms(), h, grid, observers, radius=radius, **PARAMS)[0]
        assert (part <= cnt).all() and (part < cnt).any() and (part > 0).any()
