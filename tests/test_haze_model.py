"""The haze CPU model (tests/haze_model) against what haze must do: det_exp is within its measured bound of float64 exp,
exact at 0 and monotone; both branches of the height factor agree with float64 at and around the threshold between them; hand-worked
pixels come out as worked; the scenes the GPU tests draw are part hazed, reach the clipped path and both branches; and a float64
restatement of the whole contract agrees with the model to one byte step."""

import numpy as np
import pytest

import support  # noqa: F401  (the repository root and the model directories on sys.path)
import haze_model as hzm
from overlay_scenes import CAMERAS, GRID, heights

gbm = hzm.gbm
ocm = gbm.ocm

# Measured on the sweeps below, asserted as the bounds: the largest error of det_exp against float64 exp, 1.0021 ulp; of
# the series branch of g where the contract uses it (|s| < 1/2), 1.91 ulp, and of the difference branch (|s| >= 1/2), 2.71 ulp, the latter at
# the threshold: the difference of two rounded exponentials loses a bit for every halving of s (5.9 ulp at |s| = 1/4, 40 ulp at 2^-5, which
# is why the threshold stands at 1/2 and the series runs to s^8: its truncation is below 2^-30 there).
DET_EXP_ULP = 1.01
G_SERIES_ULP = 2.0
G_DIFFERENCE_ULP = 3.0
# the share of pixels whose bytes differ from the float64 restatement, measured: none in the 24 frames of the test at the end
F64_DIFFERING_SHARE = 0.0


def ulps(got, want64):
    """|got - want| in units of the spacing of float32 at want"""
    want64 = np.asarray(want64, np.float64)
    return np.abs(np.asarray(got, np.float64) - want64) / np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)


def exp_sweep():
    xs = [np.linspace(-87.0, 16.0, 200001).astype(np.float32), np.array([-87.0, 16.0, 0.0, -0.0], np.float32)]
    xs.append(np.array([s * 2.0 ** k for k in range(-40, 7) for s in (-1.0, 1.0) if -87.0 <= s * 2.0 ** k <= 16.0], np.float32))
    half = []                                               # the reduction's half-way points (n + 1/2) ln 2 and their neighbours
    for n in range(-126, 24):
        c = np.float32((n + 0.5) * np.log(2.0))
        lo = hi = c
        half.append(c)
        for _ in range(2):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            half += [lo, hi]
    xs.append(np.array([v for v in half if -87.0 <= v <= 16.0], np.float32))
    return np.unique(np.concatenate(xs))


def test_det_exp_is_within_its_measured_bound_exact_at_zero_and_monotone():
    xs = exp_sweep()
    e = hzm.det_exp(xs)
    err = ulps(e, np.exp(xs.astype(np.float64)))
    print(f"det_exp: {len(xs)} points, largest error {err.max():.4f} ulp at x = {xs[err.argmax()]!r}")
    assert err.max() <= DET_EXP_ULP
    assert hzm.det_exp(np.float32(0.0)) == np.float32(1.0) and hzm.det_exp(np.float32(-0.0)) == np.float32(1.0)
    assert (np.diff(e.astype(np.float64)) >= 0.0).all()                                 # xs is sorted
    assert np.isfinite(e).all() and (e >= np.float32(2.0 ** -126)).all()             # neither an infinity nor a subnormal on [-87, 16]


def g64(k_e, k_p):
    """the height factor in float64 from the float32 arguments the model gets"""
    k_e, k_p = np.float32(k_e), np.float32(k_p)
    s = np.float64(np.float32(k_p - k_e))
    return np.exp(-np.float64(k_e)) * (1.0 if s == 0.0 else -np.expm1(-s) / s)


def test_both_branches_of_g_agree_with_float64_around_the_threshold():
    thr = np.float32(hzm.SERIES_BELOW)
    worst = {0: 0.0, 1: 0.0}
    fracs = list(np.linspace(0.5, 1.5, 81)) + [float(np.nextafter(np.float32(1), np.float32(0))), 1.0, float(np.nextafter(np.float32(1), np.float32(2)))]
    for k_e in (-16.0, -3.3, -0.5, 0.0, 0.7, 2.5, 7.3, 20.0, 63.0):
        for f in fracs:
            for sign in (-1.0, 1.0):
                k_p = np.float32(np.float32(k_e) + np.float32(sign * f) * thr)
                if not -16.0 <= k_p <= 64.0:
                    continue
                s = abs(np.float32(k_p - np.float32(k_e)))
                want = g64(k_e, k_p)
                b = 0 if s < thr else 1                      # each branch where the contract uses it: the series below the threshold
                worst[b] = max(worst[b], float(ulps(hzm.g_branch(k_e, k_p, b), want)))
                assert hzm.g_branch(k_e, k_p) == hzm.g_branch(k_e, k_p, b)
    print(f"g: series {worst[0]:.3f} ulp, difference {worst[1]:.3f} ulp")
    assert worst[0] <= G_SERIES_ULP and worst[1] <= G_DIFFERENCE_ULP
    # the series over its whole range, small s included, and s = 0
    for k_e in (-2.0, 0.0, 1.5):
        for s in (0.0, 1e-30, -1e-9, 3e-5, -0.01, 0.1, -0.3, 0.49):
            k_p = np.float32(np.float32(k_e) + np.float32(s))
            assert ulps(hzm.g_branch(k_e, k_p), g64(k_e, k_p)) <= G_SERIES_ULP
    assert hzm.g_branch(0.0, 0.0) == np.float32(1.0)


def test_g_tends_to_one_and_is_symmetric_in_eye_and_point():
    assert hzm.g(2.0, -0.3, None) == np.float32(1.0)
    dev = [abs(float(hzm.g(2.0, -0.3, f, 0.2)) - 1.0) for f in (1.0, 10.0, 100.0, 1e4, 1e6)]
    assert all(a > b for a, b in zip(dev, dev[1:])) and dev[-1] < 2e-6
    # the mean density along the line does not depend on its direction: E_e (1 - exp(-s)) / s = E_p (1 - exp(s)) / (-s).  On the difference
    # branch numerator and denominator only change sign, so the bits are equal; on the series the two sides are different sums
    for eye, y, f in ((2.0, -0.3, 0.3), (0.6, 0.75, 0.2), (2.2, 0.1, 1.0), (-0.4, 0.6, 0.5)):
        assert hzm.g_branch(eye / f, y / f) == hzm.g_branch(eye / f, y / f, 1)
        assert hzm.g(eye, y, f) == hzm.g(y, eye, f), (eye, y, f)
    for eye, y, f in ((2.0, -0.3, 8.0), (0.6, 0.75, 1.0), (2.2, 0.1, 50.0)):
        assert hzm.g_branch(eye / f, y / f) == hzm.g_branch(eye / f, y / f, 0)
        a, b = hzm.g(eye, y, f), hzm.g(y, eye, f)
        assert ulps(a, np.float64(b)) <= 2.0 * G_SERIES_ULP, (eye, y, f)
    # the clamps: a point far below the base and an eye far above it stay finite
    assert np.isfinite(hzm.g(1e6, -1e6, 0.01)) and hzm.g(1e6, 1e6, 0.01) == hzm.det_exp(np.float32(-64.0))


def test_hand_worked_pixels():
    ln2 = np.float32(np.log(2.0))
    # tau = fl(ln 2): a = 1 - det_exp(-fl(ln 2)).  The subtraction is exact (Sterbenz); det_exp is within DET_EXP_ULP of exp, whose value 1/2
    # moves by 1/2 |fl(ln 2) - ln 2| <= 2^-26 = 1/4 ulp of 1/2 for the rounding of the argument
    a = hzm.alpha(1.0, 0.0, 2.0, ln2)
    assert abs(float(a) - 0.5) <= (DET_EXP_ULP + 0.25) * 2.0 ** -24
    assert hzm.alpha(3.0, 0.0, 2.0, np.float32(np.log(2.0) / 2.0), start=1.0) == a      # the path starts at `start`
    # start at or beyond the pixel's depth, a non-finite depth, no density, alpha 0: untouched
    for kw in (dict(d=3.0, start=3.0), dict(d=3.0, start=4.5), dict(d=np.inf), dict(d=np.nan), dict(d=-1.0), dict(d=3.0, density=0.0),
               dict(d=3.0, rgba=(200, 215, 235, 0)), dict(d=3.0, max_opacity=0.0)):
        kw = {"d": 3.0, "y": 0.1, "eye": 2.0, "density": 0.5, **kw}
        assert hzm.alpha(**kw) == 0.0, kw
    # max_opacity caps the opacity, the colour's alpha scales it
    assert hzm.alpha(100.0, 0.0, 2.0, 1.0, max_opacity=0.35) == np.float32(0.35)
    assert hzm.alpha(100.0, 0.0, 2.0, 1.0, rgba=(1, 2, 3, 128)) == np.float32(1.0) * (np.float32(128.0) / np.float32(255.0))
    assert hzm.alpha(1e30, 0.0, 2.0, 1e30) == np.float32(1.0)                            # tau overflows: clamped at 87, a0 rounds to 1
    # height: haze that thins out upwards is thicker for a low point than for a high one, and thinner than at the base when all above it
    lo, hi = hzm.alpha(3.0, -0.5, 2.0, 0.5, falloff=0.5), hzm.alpha(3.0, 0.7, 2.0, 0.5, falloff=0.5)
    assert 0.0 < hi < lo < hzm.alpha(3.0, 0.0, 2.0, 0.5)
    # a = 1 replaces the colour by the haze colour's bytes; a = 0.5 of white over black in linear light is sRGB 188
    assert hzm.blend((10, 20, 30), (200, 215, 235, 255), 1.0) == (200, 215, 235)
    assert hzm.blend((0, 0, 0), (255, 255, 255, 255), 0.5) == (188, 188, 188)
    h = heights()
    import oracle
    W, H = 96, 64
    u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS["fill"]), np.float32).reshape(44)
    rgba, vis = oracle.render_terrain(u, W, H, GRID, h, np.zeros(1024, np.uint8), want_vis=True, nthreads=8)
    frame, a = hzm.frame(rgba, vis, u, h, GRID, 1e6, rgba=(9, 99, 199, 255))
    cov = vis != 0
    assert (a[cov] == 1.0).all() and (frame[cov] == (9, 99, 199, 255)).all() and np.array_equal(frame[~cov], rgba.reshape(H, W, 4)[~cov])
    assert hzm.eye_y(u) == np.float32(2.2) or abs(float(hzm.eye_y(u)) - 2.2) < 1e-6


@pytest.fixture(scope="module")
def oracle_frames():
    import oracle
    W, H = 96, 64
    h = heights()
    out = {}
    for cam in CAMERAS:
        u = np.array(oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *CAMERAS[cam]), np.float32).reshape(44)
        rgba, vis = oracle.render_terrain(u, W, H, GRID, h, np.arange(1024, dtype=np.uint8), want_vis=True, nthreads=8)
        out[cam] = (u, rgba.reshape(H, W, 4), vis)
    return h, out


def test_the_gpu_tests_scenes_are_part_hazed_and_reach_every_path(oracle_frames):
    h, frames = oracle_frames
    both = []
    for cam, (u, rgba, vis) in frames.items():
        cov = vis != 0
        P = hzm.SCENE_PARAMS[cam]
        frame, a = hzm.frame(rgba, vis, u, h, GRID, **P)
        part = float(((a[cov] > 0.0) & (a[cov] < 1.0)).mean())
        print(f"{cam}: {part:.3f} of the covered pixels have 0 < a < max_opacity; a up to {a.max():.3f}")
        assert cov.any() and 0.1 <= part <= 0.9, (cam, part)
        assert (a[~cov] == 0.0).all() and np.array_equal(frame[~cov], rgba[~cov])                          # background off: never touched
        assert np.array_equal(frame[a == 0.0], rgba[a == 0.0]) and (frame[a > 0.0] != rgba[a > 0.0]).any()
        capped, ac = hzm.frame(rgba, vis, u, h, GRID, max_opacity=0.35, **P)
        partc = float(((ac[cov] > 0.0) & (ac[cov] < np.float32(0.35))).mean())
        assert ac.max() == np.float32(0.35) and 0.1 <= partc <= 0.9, (cam, partc)
        sky, asky = hzm.frame(rgba, vis, u, h, GRID, max_opacity=0.8, background=True, **P)
        assert (asky[~cov] == np.float32(0.8)).all() and np.array_equal(sky[..., 3], rgba[..., 3] | np.where(asky > 0, 255, 0).astype(np.uint8) * cov)
        for f in hzm.SCENE_FALLOFFS:
            _, af, which = hzm.frame(rgba, vis, u, h, GRID, falloff=f, base=hzm.SCENE_BASE, want_branch=True, **P)
            assert (which[~cov] == -2).all() and set(np.unique(which[cov])) <= {0, 1}
            if (which == 0).any() and (which == 1).any():
                both.append((cam, f))
            partf = float(((af[cov] > 0.0) & (af[cov] < 1.0)).mean())
            assert 0.1 <= partf <= 0.9, (cam, f, partf)
        if cam == "near":
            _, clipped = ocm.terrain_q(vis, u, h, GRID)
            assert (clipped & cov & (a > 0.0)).any()                   # hazed pixels on the generic (clipped) path
    print("both branches of g in one frame:", both)
    assert ("near", 0.3) in both and ("default", 4.0) in both and ("fill", 4.0) in both
    assert not any(f == 50.0 for _, f in both) and ("default", 0.3) not in both


# ---- the whole contract again in float64 numpy ----

def eotf64(s):
    s = np.asarray(s, np.float64)
    return np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)


def frame64(rgba, vis, u, depth, y, density, rgba_haze=hzm.DEFAULTS["rgba"], start=0.0, falloff=None, base=0.0, max_opacity=1.0, background=False):
    """depth and y are the geometry-buffer model's planes (float32): what the contract's item 1 names; everything after it in float64"""
    cov = vis != 0
    d, y = depth.astype(np.float64), y.astype(np.float64)
    eye = -(np.float64(u[4]) * u[12] + np.float64(u[5]) * u[13] + np.float64(u[6]) * u[14])
    with np.errstate(all="ignore"):
        path = np.maximum(d - start, 0.0)
        if falloff is None:
            g = 1.0
        else:
            k_e, k_p = np.clip((eye - base) / falloff, -16.0, 64.0), np.clip((y - base) / falloff, -16.0, 64.0)
            s = k_p - k_e
            g = np.exp(-k_e) * np.where(s == 0.0, 1.0, -np.expm1(-s) / np.where(s == 0.0, 1.0, s))
        a = np.minimum(-np.expm1(-np.minimum(density * path * g, 87.0)), max_opacity) * (rgba_haze[3] / 255.0)
    a = np.where(cov, np.where(np.isfinite(d) & (path > 0.0), a, 0.0), max_opacity * (rgba_haze[3] / 255.0) if background else 0.0)
    a = np.where(a > 0.0, a, 0.0)
    lin = eotf64(rgba[..., :3] / 255.0)
    out = eotf64(np.array(rgba_haze[:3]) / 255.0) * a[..., None] + lin * (1.0 - a[..., None])
    thr = eotf64((np.arange(1, 256) - 0.5) / 255.0)
    frame = rgba.copy()
    frame[..., :3] = np.searchsorted(thr, out, side="right").astype(np.uint8)
    frame[..., 3] = np.where((a > 0.0) & cov, 255, rgba[..., 3])
    frame[a == 0.0] = rgba[a == 0.0]
    return frame, a


def test_a_float64_restatement_agrees_to_one_byte_step(oracle_frames):
    h, frames = oracle_frames
    worst_share = 0.0
    for cam, (u, rgba, vis) in frames.items():
        depth, position, _ = gbm.planes(vis, u, h, GRID)
        P = hzm.SCENE_PARAMS[cam]
        cases = [dict(P), dict(P, start=0.0), dict(P, max_opacity=0.35), dict(P, rgba=(255, 120, 40, 128)), dict(P, max_opacity=0.8, background=True)]
        cases += [dict(P, falloff=f, base=hzm.SCENE_BASE) for f in hzm.SCENE_FALLOFFS]
        for kw in cases:
            frame, a = hzm.frame(rgba, vis, u, h, GRID, **kw)
            kw64 = dict(kw)
            col = kw64.pop("rgba", hzm.DEFAULTS["rgba"])
            want, a64 = frame64(rgba, vis, u, depth, position[..., 1], rgba_haze=col, **kw64)
            # a few ulp in a move the linear colour by about 1e-6, far below the smallest byte step
            assert np.abs(a.astype(np.float64) - a64).max() <= 8.0 * 2.0 ** -24, (cam, kw)
            diff = np.abs(frame.astype(np.int16) - want.astype(np.int16))
            assert diff.max() <= 1, (cam, kw)
            worst_share = max(worst_share, float((diff.max(axis=-1) > 0).mean()))
    print(f"largest share of pixels that differ from the float64 restatement (by one step): {worst_share:.5f}")
    assert worst_share <= F64_DIFFERING_SHARE
