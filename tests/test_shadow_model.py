"""The cast-shadow CPU model (tests/shadow_model) against what shadows must do: flat ground is lit, a ridge casts a strip
of the right length, the field commutes with the grid's symmetries exactly, a higher sun never darkens a vertex, a float64 march
along the same lines agrees, non-finite heights neither cast nor take a shadow, and the scene the GPU tests draw is part in shadow."""

import numpy as np
import pytest

from support import bits, smooth
import shadow_model as shm
from overlay_scenes import CAMERAS, GRID, heights

SUNS = [(0.9, 0.5, 0.31), (0.31, 0.5, 0.9), (-0.31, 0.4, 0.9), (-0.9, 0.7, 0.31), (-0.9, 0.3, -0.31), (-0.31, 0.6, -0.9), (0.31, 0.45, -0.9), (0.9, 0.55, -0.31),
        (1.0, 0.6, 0.0), (-1.0, 0.6, 0.0), (0.0, 0.6, 1.0), (0.0, 0.6, -1.0), (0.5, 0.4, 0.5), (-0.5, 0.4, 0.5), (0.5, 0.4, -0.5), (-0.5, 0.4, -0.5),
        (0.0, 1.0, 0.0), (0.7, 0.0, 0.2), (0.2, -0.3, 0.7)]


def test_flat_terrain_is_lit():
    for level in (0.0, 0.37, -2.0):
        h = np.full((65, 65), level, np.float32)
        for sun in SUNS:
            assert (shm.field_heights(h, sun) == 1.0).all(), (level, sun)


@pytest.mark.parametrize("theta", [15.0, 30.0, 55.0])
@pytest.mark.parametrize("axis", ["x", "z"])
def test_a_ridge_casts_a_strip_of_the_right_length(theta, axis):
    n, R, row = 257, 0.2, 200
    spacing = 2.0
    h = np.zeros((n, n), np.float32)
    h[row, :] = R
    sun = (0.0, np.sin(np.radians(theta)), np.cos(np.radians(theta)))     # from +z, perpendicular to the ridge
    if axis == "x":
        h, sun = h.T.copy(), sun[::-1]
    lit = shm.field_heights(h, sun, spacing=spacing, strength=1.0, softness=1e-9, bias=1e-5)
    lit = lit.T if axis == "x" else lit
    cell = 3.0 / (n - 1) * spacing
    length = R / np.tan(np.radians(theta)) / cell                         # in cells
    assert (lit[row:, :] == 1.0).all()                                    # the ridge and the sun side
    dark = (lit[:row, :] == 0.0)
    assert (dark == dark[:, :1]).all() and ((lit == 0.0) | (lit == 1.0)).all()
    count = int(dark[:, 0].sum())
    assert dark[row - count:row, 0].all()                                 # one strip, against the ridge
    assert abs(count - length) <= 1.0, (count, length)


def test_the_field_commutes_with_the_symmetries_of_the_grid():
    n, exag, P = 97, 1.3, shm.DEFAULTS
    h = smooth(n, 3)
    for sun in SUNS:
        sx, sy, sz = sun
        f = shm.field_heights(h, sun, exag=exag)
        ft = shm.field_heights(h.T.copy(), (sz, sy, sx), exag=exag)
        if abs(sx) != abs(sz) or sx == 0.0:                  # (no horizontal component: everything is lit, in both)
            assert np.array_equal(bits(ft), bits(f.T)), sun
        else:
            # An exact tie takes x as the major axis in both problems: the same diagonals, but a vertex's step number k differs by
            # its line's offset between them, so y + k d rounds differently -- equal as reals, not bit for bit.
            # Each problem's excess e lies within 20 ulp of T + bias of the exact one (the float64 test below derives that), so the
            # two differ by at most twice that; lit = 1 - strength clamp((e - bias) / softness) passes the difference on times
            # strength / softness, and its own division, product and difference add an ulp of 1 each, in either problem.
            d = 3.0 / (n - 1) * max(sy, 0.0) / abs(sx)
            T = float(np.abs(h.astype(np.float64) * exag).max()) + n * d
            bound = 2.0 * 20.0 * 2.0 ** -24 * (T + P["bias"]) * P["strength"] / P["softness"] + 2.0 * 3.0 * 2.0 ** -24
            assert np.abs(ft.astype(np.float64) - f.T).max() <= bound, (sun, np.abs(ft.astype(np.float64) - f.T).max(), bound)
        assert np.array_equal(bits(shm.field_heights(h[:, ::-1].copy(), (-sx, sy, sz), exag=exag)), bits(f[:, ::-1])), sun
        assert np.array_equal(bits(shm.field_heights(h[::-1, :].copy(), (sx, sy, -sz), exag=exag)), bits(f[::-1, :])), sun
    assert (shm.field_heights(h, SUNS[0], exag=exag) < 1).any()


@pytest.mark.parametrize("axis", ["x", "z"])
@pytest.mark.parametrize("phi", [25.0, -25.0, 40.0])
def test_an_oblique_sun_throws_the_shadow_of_a_ridge_sideways(phi, axis):
    """a ridge segment in a row, the sun phi degrees off its normal: the shadow is the parallelogram swept from the segment along the
    sun's horizontal direction -- row m behind the ridge is dark between the segment's ends moved m tan(phi) cells along the ridge,
    as far as the ray's run R / tan(theta) reaches.  This pins the direction of the shear, which the float64 march (it takes its
    lines from the same rule) cannot.  Tolerance: a line lies up to half a cell off the ray, its ends are whole cells: 1.5 cells."""
    n, R, row, c0, c1, theta = 257, 0.25, 200, 100, 160, 30.0
    h = np.zeros((n, n), np.float32)
    h[row, c0:c1 + 1] = R
    t, p = np.radians(theta), np.radians(phi)
    sun = (np.sin(p) * np.cos(t), np.sin(t), np.cos(p) * np.cos(t))       # from +z, turned towards +x by phi
    if axis == "x":
        h, sun = h.T.copy(), sun[::-1]
    lit = shm.field_heights(h, sun, spacing=1.0, strength=1.0, softness=1e-9, bias=1e-5)
    lit = lit.T if axis == "x" else lit
    cell = 3.0 / (n - 1)
    reach = R / np.tan(t) * np.cos(p) / cell                              # rows behind the ridge the shadow reaches
    assert (lit[row:, :] == 1.0).all()
    checked = 0
    for m in range(2, int(reach) - 1):
        dark = np.flatnonzero(lit[row - m, :] == 0.0)
        assert len(dark) and (np.diff(dark) == 1).all(), m
        shift = m * np.tan(p)
        assert abs(dark[0] - (c0 - shift)) <= 1.5 and abs(dark[-1] - (c1 - shift)) <= 1.5, (m, dark[0], dark[-1], shift)
        checked += 1
    assert checked >= 5 and abs(checked * np.tan(p)) > 2.0                # (the sideways throw is more than the tolerance)
    assert (lit[:row - int(reach) - 2, :] == 1.0).all()


@pytest.mark.parametrize("horizontal", [(0.9, 0.31), (-0.31, 0.9), (1.0, 0.0), (0.0, -1.0), (0.5, 0.5), (-0.7, -0.2)])
def test_raising_the_sun_never_darkens_a_vertex(horizontal):
    """fixed azimuth: the horizontal components stay as they are, the elevation sets the vertical one -- the lines and d's
    denominator are then the same at every elevation, and d grows with the elevation"""
    h = smooth(129, 5)
    assert np.isfinite(h).all()
    sx, sz = horizontal
    r = np.hypot(sx, sz)
    last = None
    for el in (-10.0, 0.0, 2.0, 5.0, 10.0, 20.0, 30.0, 45.0, 60.0, 75.0, 85.0, 89.0):
        f = shm.field_heights(h, (sx, r * np.tan(np.radians(el)), sz), strength=0.7, softness=0.02, bias=0.002)
        if last is not None:
            assert (f >= last).all(), (horizontal, el, int((f < last).sum()))
        last = f
    assert (shm.field_heights(h, (sx, r * np.tan(np.radians(5.0)), sz)) < 1).any()


def brute_force_excess(h, sun, spacing, exag):
    """float64 march over the same sheared lines: the excess e_k at every vertex (-inf at a line's first vertex)"""
    n = h.shape[0]
    sx, sy, sz = (np.float32(v) for v in sun)
    zmajor = abs(sz) > abs(sx)
    smaj, smin = (sz, sx) if zmajor else (sx, sz)
    a = np.float32(abs(smin)) / np.float32(abs(smaj))                      # (binary32: which vertices a line holds is part of the contract)
    d = (3.0 / (n - 1)) * spacing * max(float(sy), 0.0) / abs(float(smaj))
    s = -1 if smin < 0 else 1
    shear = np.rint(np.arange(n, dtype=np.float32) * a).astype(np.int64)
    y = h.astype(np.float64) * exag
    e = np.full((n, n), -np.inf)
    for c in range(-n, 2 * n):
        run = -np.inf
        for k in range(n):
            minor = c - s * shear[k]
            if not 0 <= minor < n:
                continue
            major = n - 1 - k if smaj > 0 else k
            j, i = (major, minor) if zmajor else (minor, major)
            e[j, i] = run - k * d - y[j, i]
            run = max(run, y[j, i] + k * d)
    return e, d


@pytest.mark.parametrize("sun", SUNS[:16])
def test_a_float64_march_over_the_same_lines_agrees(sun):
    n, spacing, exag, bias, strength = 48, 1.5, 1.2, 0.004, 0.6
    h = smooth(n, 11) * np.float32(3.0)
    lit = shm.field_heights(h, sun, spacing=spacing, exag=exag, strength=strength, softness=1e-12, bias=bias)
    e, d = brute_force_excess(h, sun, spacing, exag)
    # binary32 against exact: y = h exag (1 rounding of a value below Y), k d with d itself three roundings off (5 ulp of n d), the
    # sum y + k d, M - k d, the difference with y and with the bias (1 ulp each of a value below 3 T, T = Y + n d): below 20 ulp of T + bias
    T = float(np.abs(h.astype(np.float64) * exag).max()) + n * d
    margin = 20.0 * 2.0 ** -24 * (T + bias)
    decided = np.abs(e - bias) > margin
    assert (~decided).mean() <= 0.01, (~decided).mean()
    want = np.where(e > bias, np.float32(1.0) - np.float32(strength), np.float32(1.0)).astype(np.float32)
    assert np.array_equal(lit[decided], want[decided]), int((lit[decided] != want[decided]).sum())
    assert (want[decided] < 1).any()


def test_non_finite_heights_cast_nothing_and_are_lit():
    h = smooth(65, 2)
    for sun in SUNS[:12]:
        for bad in (np.nan, np.inf, -np.inf):
            g, low = h.copy(), h.copy()
            g[20, 30] = g[40, 41] = bad
            low[20, 30] = low[40, 41] = -1e30                              # a pit casts nothing either
            f, want = shm.field_heights(g, sun), shm.field_heights(low, sun)
            assert f[20, 30] == 1.0 and f[40, 41] == 1.0
            want[20, 30] = want[40, 41] = 1.0
            assert np.array_equal(bits(f), bits(want)), (sun, bad)
    g = np.full((33, 33), np.nan, np.float32)
    assert (shm.field_heights(g, SUNS[0]) == 1.0).all()
    # the first vertex of every line is lit, whatever it is
    f = shm.field_heights(smooth(65, 2) - 5.0, (1.0, 0.01, 0.0))
    assert (f[:, -1] == 1.0).all()


@pytest.mark.parametrize("size", [(1920, 1080), (257, 131)])
def test_the_gpu_tests_scene_is_part_in_shadow(size):
    import oracle
    W, H = size
    h = heights()
    lut = np.zeros(1024, np.uint8)
    for cam in CAMERAS:
        u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam]), np.float32).reshape(44)
        u[32:35] = shm.sun_vector(*shm.SCENE_SUN_DEG)
        rgba, vis = oracle.render_terrain(u, W, H, GRID, h, lut, want_vis=True, nthreads=8)
        lit = shm.field(u, h, GRID, **shm.SCENE_PARAMS)
        frame, shadowed = shm.frame(rgba, vis, u, h, GRID, lut, lit)
        covered = int((vis != 0).sum())
        frac = shadowed.sum() / covered
        assert covered > 0 and 0.1 <= frac <= 0.9, (cam, size, frac)
        assert not shadowed[vis == 0].any()
        assert np.array_equal(frame[~shadowed], rgba.reshape(H, W, 4)[~shadowed])
