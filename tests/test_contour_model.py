"""The contour CPU model (tests/contour_model) against the contract's four rules, restated here in Python: records bit
for bit and in order, the chaining of segments into closed joints, the interpolated height of every crossing point, and the segment
count against an independent numpy count -- on random, ramp and plateau-on-a-level surfaces, on grids whose cell count is and is not a
multiple of 8.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

import support  # noqa: F401  (the repository root and the model directories on sys.path)
import contour_model as cm

F = np.float32
U = 2.0 ** -24                                                # unit roundoff of binary32


def fma32(a, b, c):
    """fma(a, b, c) in binary32, rounded once: exact in rationals, then to the nearest float (ties to even)"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    f = F(float(exact))                                       # (float(Fraction) is correctly rounded to binary64; binary32 comes next)
    best = None
    for cand in (np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))):
        d = abs(Fraction(float(cand)) - exact)
        even = (int(F(cand).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, F(cand))
    return best[1]


def surfaces(n, seed=3):
    """name -> (n, n) float32 surface h[j, i]; levels"""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rnd = (rng.random((n, n)) * 0.6 - 0.3).astype(F)
    ramp = (0.01 * ii + 0.003 * jj - 0.2).astype(F)
    plateau = rnd.copy()
    plateau[n // 4:n // 2, n // 3:2 * n // 3] = F(0.125)      # a plateau lying exactly on a level
    plateau[5, 5] = F(-0.125)                                 # a single vertex exactly on another
    lv = np.array([-0.25, -0.125, 0.0, 0.125, 0.25], F)
    return {"random": (rnd, lv), "ramp": (ramp, np.arange(-0.2, 1.5, 0.0625).astype(F)), "plateau": (plateau, lv)}


def python_model(h, spacing, levels):
    """rules 1-4 in Python -> per segment (level index, p0 (x, z), p1 (x, z), the two edges ((hP, hQ, t), ...))"""
    n = h.shape[0]
    nm1, nb = n - 1, (n - 1 + 7) // 8
    step = F(3.0) / (F(n) - F(1.0))
    X = [(F(-1.5) + F(i) * step) * F(spacing) for i in range(n)]
    out = []

    def cross(L, P, Q):
        t = (L - P[2]) / (Q[2] - P[2])
        return (fma32(t, Q[0] - P[0], P[0]), fma32(t, Q[1] - P[1], P[1])), (P[2], Q[2], t)

    for b in range(nb * nb):
        for cell in range(64):
            i, j = (b % nb) * 8 + cell % 8, (b // nb) * 8 + cell // 8
            if i >= nm1 or j >= nm1:
                continue
            a, bb = (X[i], X[j], h[j, i]), (X[i + 1], X[j], h[j, i + 1])
            c, d = (X[i], X[j + 1], h[j + 1, i]), (X[i + 1], X[j + 1], h[j + 1, i + 1])
            for tri in ((a, c, bb), (bb, c, d)):
                if not all(np.isfinite(v[2]) for v in tri):
                    continue
                for k, L in enumerate(levels):
                    above = [v[2] >= L for v in tri]
                    if sum(above) in (0, 3):
                        continue
                    s = above.index(sum(above) == 1)
                    S, N, R = tri[s], tri[(s + 1) % 3], tri[(s + 2) % 3]
                    if above[s]:
                        (p0, e0), (p1, e1) = cross(L, N, S), cross(L, R, S)
                    else:
                        (p0, e0), (p1, e1) = cross(L, S, R), cross(L, S, N)
                    out.append((k, p0, p1, (e0, e1)))
    return out


@pytest.mark.parametrize("n", [41, 25])                       # 40 cells = 5 blocks; 24 + border handling at 41; 24 = 3 blocks
@pytest.mark.parametrize("name", ["random", "ramp", "plateau"])
def test_records_equal_the_rules_restated_in_python(name, n):
    h, lv = surfaces(n)[name]
    spacing = 1.0 if n == 41 else 0.7
    want = python_model(h, spacing, lv)
    for join in ("round", "none"):
        recs, nseg = cm.extract(h, spacing, lv, width_px=3.0, rgba=(1, 2, 3, 200), lift=0.02, join=join, feature=7)
        assert nseg == len(want) > 0
        seg = recs[::2] if join == "round" else recs
        assert len(seg) == nseg
        p0 = np.array([w[1] for w in want], F)
        p1 = np.array([w[2] for w in want], F)
        assert np.array_equal(seg["p0"][:, [0, 2]].view(np.uint32), p0.view(np.uint32))      # rule 4's order, rules 2 and 3's bits
        assert np.array_equal(seg["p1"][:, [0, 2]].view(np.uint32), p1.view(np.uint32))
        assert (seg["flags"] == (cm.om.SEGMENT | cm.om.DRAPE)).all()
        assert (recs["p0"][:, 1] == F(0.02)).all() and (recs["p1"][:, 1] == F(0.02)).all()
        assert (recs["size"] == F(1.5)).all() and (recs["feature"] == 7).all() and (recs["pad"] == 0).all()
        assert (recs["rgba"] == (1 | 2 << 8 | 3 << 16 | 200 << 24)).all()
        if join == "round":
            disc = recs[1::2]
            assert (disc["flags"] == (cm.om.CIRCLE | cm.om.DRAPE)).all()
            assert np.array_equal(disc["p0"], seg["p0"]) and np.array_equal(disc["p1"], seg["p0"])
    occ, _ = cm.extract(h, spacing, lv, occlude=True, depth_bias=0.05)
    assert (occ["flags"] & cm.ocm.OCCLUDE).all() and (occ["pad"][:, 0] == cm.ocm.kb_bits(0.05)).all()
    fast, nfast = cm.extract(h, spacing, lv, width_px=3.0, rgba=(1, 2, 3, 200), lift=0.02, join="none", feature=7, bracket=True)
    assert nfast == nseg and np.array_equal(fast, recs)       # the bracketed search skips nothing that crosses


@pytest.mark.parametrize("n", [100, 257])                     # grid 100: 99 cells (not a multiple of 8); grid 257: 256 cells (one)
@pytest.mark.parametrize("name", ["random", "ramp", "plateau"])
def test_segments_chain_and_count(name, n):
    """Rule 2: every interior crossing point of a level is the p1 of as many segments as it is the p0 of (so a disc at each p0
    closes every joint); where no vertex lies exactly on the level: of exactly one each.  The count equals a numpy count of
    (triangle, level) pairs."""
    h, lv = surfaces(n)[name]
    spacing = 1.0
    step = F(3.0) / (F(n) - F(1.0))
    edge = {float(F(-1.5) * F(spacing)), float((F(-1.5) + F(n - 1) * step) * F(spacing))}
    # numpy count: a level crosses a triangle iff min h < L <= max h (some vertex below, some at or above)
    a, b, c, d = h[:-1, :-1], h[:-1, 1:], h[1:, :-1], h[1:, 1:]
    total = 0
    for tri in ((a, c, b), (b, c, d)):
        st = np.stack(tri)
        for L in lv:
            total += int(((st.min(axis=0) < L) & (st.max(axis=0) >= L)).sum())
    nall = 0
    for L in lv:
        recs, nseg = cm.extract(h, spacing, [L], join="none")
        nall += nseg
        if not nseg:
            continue
        key = lambda p: p[:, [0, 2]].copy().view(np.uint64).ravel()     # noqa: E731  (x and z bits as one word)
        k0, k1 = key(recs["p0"]), key(recs["p1"])
        inner = lambda p: ~(np.isin(p[:, 0], list(edge)) | np.isin(p[:, 2], list(edge)))     # noqa: E731
        u0, c0 = np.unique(k0[inner(recs["p0"])], return_counts=True)
        u1, c1 = np.unique(k1[inner(recs["p1"])], return_counts=True)
        assert np.array_equal(u0, u1) and np.array_equal(c0, c1), f"level {L}: open joints"
        if not (h == L).any():
            assert (c0 == 1).all()
    assert nall == total > 0
    assert cm.extract(h, spacing, lv, join="none")[1] == total


def test_crossing_points_lie_on_their_level():
    """Rule 3: t = fl(fl(L - hP) / fl(hQ - hP)) carries three roundings, each a relative error of at most u = 2^-24, so
    t (hQ - hP) = (L - hP) (1 + e), |e| <= 3u + O(u^2); with |L - hP| <= |hQ - hP| the interpolated height hP + t (hQ - hP), evaluated
    exactly, is within (3u + 4u^2) |hQ - hP| of L."""
    for name in ("random", "ramp", "plateau"):
        h, lv = surfaces(41)[name]
        worst = 0.0
        for k, _p0, _p1, edges in python_model(h, 1.0, lv):
            for hP, hQ, t in edges:
                assert hP < lv[k] <= hQ and 0.0 < t <= 1.0
                err = abs(Fraction(float(hP)) + Fraction(float(t)) * (Fraction(float(hQ)) - Fraction(float(hP))) - Fraction(float(lv[k])))
                bound = Fraction(3 * U + 4 * U * U) * (Fraction(float(hQ)) - Fraction(float(hP)))
                assert err <= bound, (name, float(err), float(bound))
                worst = max(worst, float(err / (Fraction(float(hQ)) - Fraction(float(hP)))) / U)
        print(f"{name}: worst |h - L| / |hQ - hP| = {worst:.3f} u")


def test_non_finite_heights_emit_nothing_and_stay_out_of_the_bounds():
    h, lv = surfaces(41)["random"]
    h = h.copy()
    h[10, 10], h[20, 3], h[30, 30] = np.nan, np.inf, -np.inf
    want = python_model(h, 1.0, lv)
    recs, nseg = cm.extract(h, 1.0, lv, join="none")
    assert nseg == len(want) and np.isfinite(recs["p0"]).all() and np.isfinite(recs["p1"]).all()
    clean, nclean = cm.extract(surfaces(41)["random"][0], 1.0, lv, join="none")
    assert nseg < nclean
    fin = h[np.isfinite(h)]
    assert cm.bounds(h) == (float(fin.min()), float(fin.max()))
    assert cm.bounds(np.full((4, 4), np.nan, F)) == (float("inf"), float("-inf"))


def test_surface_is_the_overlay_models_vertex_height():
    tex = surfaces(33)["random"][0]
    s = cm.surface(tex, 50)
    for i, j in ((0, 0), (49, 49), (7, 31), (20, 0)):
        assert s[j, i] == F(cm.om.vertex_height(tex, 50, i, j))


def test_contour_layers_append_to_the_other_models_layers():
    tex = surfaces(33)["random"][0]
    u = np.zeros(44, F)
    u[36] = 1.0
    L = cm.Layers()
    L.points(np.zeros((3, 3), F))
    L.contours(tex, 50, u, [0.0, 0.1], width_px=5.0, join="none", occlude=True, depth_bias=0.02)
    L.lines([np.array([[0, 0, 0], [1, 0, 1]], F)])
    r = L.array()
    ct = r[r["feature"] == 3]
    assert len(ct) == L.nsegments and (ct["flags"] == (cm.om.SEGMENT | cm.om.DRAPE | cm.ocm.OCCLUDE)).all()
    assert (ct["pad"][:, 0] == cm.ocm.kb_bits(0.02)).all() and r["feature"].max() == 4
    L.set_occlusion(1, False)
    assert not (L.array()["flags"] & cm.ocm.OCCLUDE).any()
