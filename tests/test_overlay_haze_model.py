"""The hazed-overlay CPU model (tests/overlay_haze_model) against the contract of DESIGN.md 4r: the restated opacity equals the haze
model's bit for bit, a hand-worked pixel, a receding segment, depth and height at the pixel against float64, the primitive that speaks
for a feature, a near-clipped end, the stencil, layers without the flag -- and, for every (camera, size, setting) of
tests/test_gpu_overlay_haze.py, the conditions that keep its comparison from being vacuous.  No GPU needed."""

import numpy as np
import pytest

from support import bits
import haze_model as hzm
import oracle
import overlay_haze_model as ohm
import overlay_haze_scenes as sc

ocm, om = ohm.ocm, ohm.om
GRID = sc.GRID
F32 = np.float32


def uniforms(cam, W, H):
    return oracle.look_at_uniforms(oracle.KIND_SCENE, W, H, *sc.CAMERAS[cam])


def flat(W, H, colour=(10, 200, 30, 255)):
    """a flat frame and a visibility without terrain (nothing occludes)"""
    return np.broadcast_to(np.array(colour, np.uint8), (H, W, 4)).copy(), np.zeros((H, W), np.uint32)


def layers_of(calls, haze=None):
    """overlay_scenes.apply's model half; haze: None as the calls say, else every layer's flag"""
    L = ohm.Layers()
    for meth, args, kw in calls:
        kw = dict(kw) if haze is None else dict(kw, haze=haze)
        if meth == "add_points":
            L.points(args[0], **kw)
        else:
            L.lines(args[0], **kw)
    return L


# ---- the opacity function ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(sc.settings("default")))
def test_the_restated_opacity_equals_the_haze_models_bit_for_bit(name):
    kw = sc.settings("near")[name]
    rng = np.random.default_rng(5)
    n = 10000
    d = np.concatenate([rng.uniform(0.0, 12.0, n - 6), [0.0, kw["start"], np.nextafter(F32(kw["start"]), F32(9)), 1e30, np.inf, np.nan]]).astype(F32)
    y = np.concatenate([rng.uniform(-1.0, 3.0, n - 6), [0.6, 0.6, 0.6, 0.0, 0.0, 0.0]]).astype(F32)
    for eye in (F32(0.6), F32(2.2)):
        got = ohm.alpha(d, y, eye, **kw)
        want = np.array([hzm.alpha(d[k], y[k], eye, **kw) for k in range(n)], F32)
        assert np.array_equal(bits(got), bits(want)), name
        assert (got > 0).sum() > n // 2


# ---- a hand-worked pixel ------------------------------------------------------------------------------

def test_a_hand_worked_pixel():
    W, H = 96, 64
    h = sc.heights()
    u = uniforms("default", W, H)
    frame, vis = flat(W, H)
    haze = dict(density=0.6, start=1.0, rgba=(200, 215, 235, 255))
    colour = (250, 30, 60, 255)
    # the camera looks at the origin: a free point there lies on the axis, at the frame's centre -- the corner of pixels (47..48, 31..32);
    # a 6-px circle covers the centre of pixel (48, 32), 0.71 px away, whole.  Its depth is its clip-space w (float64 here).
    L = ohm.Layers().points(np.zeros((1, 3), F32), size_px=6.0, rgba=colour, haze=True)
    out, ah, touch = ohm.composite(frame, vis, u, h, GRID, L, haze=haze, want_planes=True)
    d = (u[16:32].reshape(4, 4).T.astype(np.float64) @ u[0:16].reshape(4, 4).T.astype(np.float64) @ np.array([0.0, 0.0, 0.0, 1.0]))[3]
    assert 4.0 < d < 8.0
    P = ohm.probe(W, H, u, h, GRID, L.array()[0], 48, 32, haze)
    assert P["cover"] == 1.0 and abs(P["d"] - d) < 1e-5 * d and P["y"] == 0.0
    a = hzm.alpha(F32(d), 0.0, hzm.eye_y(u), **haze)
    assert abs(a - (1.0 - np.exp(-0.6 * (d - 1.0)))) < 1e-6 and abs(float(ah[32, 48]) - float(a)) < 1e-6 and touch[32, 48]
    # item 4: the point's colour under the haze (haze_model.blend's arithmetic), then over the pixel with coverage 1 and alpha 1
    hazed = hzm.blend(colour[:3], haze["rgba"], a)
    lin = [F32(om.decode(haze["rgba"][k])) * F32(a) + F32(om.decode(colour[k])) * (F32(1.0) - F32(a)) for k in range(3)]
    assert tuple(om.encode(v) for v in lin) == hazed
    one = F32(1.0)
    want = tuple(om.encode(lin[k] * one + F32(om.decode(frame[32, 48, k])) * (one - one)) for k in range(3))
    assert tuple(int(v) for v in out[32, 48, :3]) == want == hazed
    assert hazed != colour[:3] and out[32, 48, 3] == 255
    plain = ohm.composite(frame, vis, u, h, GRID, L)
    assert tuple(int(v) for v in plain[32, 48, :3]) == colour[:3]


# ---- depth and height along a segment ---------------------------------------------------------------------

def covered(W, H, u, h, rec, haze):
    """[(px, py, probe)] of the pixels one record covers"""
    out = []
    for py in range(H):
        for px in range(W):
            P = ohm.probe(W, H, u, h, GRID, rec, px, py, haze)
            if P["cover"] > 0:
                out.append((px, py, P))
    return out


def test_the_opacity_does_not_decrease_along_a_receding_segment():
    W, H = 96, 64
    h = sc.heights()
    u = uniforms("default", W, H)
    haze = sc.settings("default")["uniform"]
    rec = ohm.Layers().lines([sc.LONG_SEGMENT], width_px=1.0, cap="butt", haze=True).array()[0]
    px = covered(W, H, u, h, rec, haze)
    assert len(px) > 40
    P0 = px[0][2]
    sign = 1.0 if P0["rw_b"] < P0["rw_a"] else -1.0            # t runs away from the eye, or towards it
    px.sort(key=lambda e: sign * e[2]["t"])
    ds = np.array([e[2]["d"] for e in px])
    ah = np.array([e[2]["ah"] for e in px])
    assert (np.diff(ds) >= 0).all() and ds[-1] > ds[0] + 3.0
    assert (np.diff(ah) >= 0).all() and ah[0] == 0.0 and ah[-1] > 0.8          # clear before `start`, mostly haze at the far end


def f64_segment(u, W, H, p0, p1, y0, y1):
    """float64 restatement of item 1: -> f(px, py) = (d, y) at a pixel centre, for the segment p0 -> p1 with world heights y0, y1"""
    V, Pm = u[0:16].reshape(4, 4).T.astype(np.float64), u[16:32].reshape(4, 4).T.astype(np.float64)
    ends = []
    for p, y in ((p0, y0), (p1, y1)):
        c = Pm @ (V @ np.array([p[0], y, p[2], 1.0], np.float64))
        ends.append([c, float(y)])
    (a, ya), (b, yb) = ends
    for plane in range(2):
        da, db = (a[2], b[2]) if plane == 0 else (a[3] - a[2], b[3] - b[2])
        if (da >= 0) and (db >= 0):
            continue
        assert da >= 0 or db >= 0
        if da >= 0:
            t = da / (da - db)
            b, yb = a + t * (b - a), ya + t * (yb - ya)
        else:
            t = db / (db - da)
            a, ya = b + t * (a - b), yb + t * (ya - yb)
    rwa, rwb = 1.0 / a[3], 1.0 / b[3]
    sa = np.array([(a[0] * rwa + 1) * W / 2, (1 - a[1] * rwa) * H / 2])
    sb = np.array([(b[0] * rwb + 1) * W / 2, (1 - b[1] * rwb) * H / 2])
    e = sb - sa
    Ln = np.hypot(*e)

    def at(px, py):
        t = min(max(np.dot(np.array([px + 0.5, py + 0.5]) - sa, e / Ln) / Ln, 0.0), 1.0)
        rw = rwa + t * (rwb - rwa)
        return 1.0 / rw, (ya * rwa + t * (yb * rwb - ya * rwa)) / rw
    return at, (ya, yb)


# the largest differences of the binary32 contract from float64 over the segments below, as measured and rounded up:
# relative in d, absolute in y (world units; the heights here lie within +-1).  `near` holds the segment that starts in the eye itself,
# whose clipped end takes a t of nearly 1 of a difference of nearly equal numbers.
F64_MAX = {"default": (2e-7, 2e-7), "fill": (2e-7, 2e-7), "near": (5e-6, 1.1e-6)}


@pytest.mark.parametrize("cam", sc.CAMS)
def test_depth_and_height_at_the_pixel_against_float64(cam):
    W, H = 96, 64
    h = sc.heights()
    u = uniforms(cam, W, H)
    haze = sc.settings(cam)["falloff 4.0"]
    exag = float(u[38])
    worst_d = worst_y = 0.0
    n = 0
    for drape in (False, True):
        paths = [sc.LONG_SEGMENT * F32([1, 0.2 if drape else 1, 1]), np.array([[1.2, 0.05, -0.3], [-0.9, 0.3, 1.3]], F32), sc.NEAR_PATH[2:4],
                 np.array([[0.5, 0.3, 0.2], [1.5, 0.1, 1.4]], F32)]
        for rec in ohm.Layers().lines(paths, width_px=1.0, cap="butt", drape=drape, haze=True).array():
            p0, p1 = rec["p0"].astype(np.float64), rec["p1"].astype(np.float64)
            y0, y1 = ((float(om.drape(u, h, GRID, p[0], p[2])) * exag + p[1] if drape else p[1]) for p in (p0, p1))
            px = covered(W, H, u, h, rec, haze)
            if not px:
                continue
            at, _ = f64_segment(u, W, H, p0, p1, y0, y1)
            for x, y, P in px:
                d64, y64 = at(x, y)
                worst_d = max(worst_d, abs(float(P["d"]) - d64) / d64)
                worst_y = max(worst_y, abs(float(P["y"]) - y64))
                n += 1
    print(f"{cam}: {n} pixels, max |d - d64| / d64 = {worst_d:.3g}, max |y - y64| = {worst_y:.3g}")
    assert n > 50
    assert worst_d <= F64_MAX[cam][0] and worst_y <= F64_MAX[cam][1], (worst_d, worst_y)


def test_a_near_clipped_end_takes_the_interpolated_height():
    W, H = 96, 64
    h = sc.heights()
    u = uniforms("near", W, H)
    haze = sc.settings("near")["uniform"]
    seg = sc.NEAR_PATH[2:4]                                       # from the eye itself out across the terrain: the end at the eye is clipped
    rec = ohm.Layers().lines([seg], width_px=1.0, cap="butt", haze=True).array()[0]
    P = ohm.probe(W, H, u, h, GRID, rec, 0, 0, haze)
    _, (ya, yb) = f64_segment(u, W, H, seg[0].astype(np.float64), seg[1].astype(np.float64), float(seg[0][1]), float(seg[1][1]))
    assert P["y_b"] == seg[1][1]                                  # the end that was not clipped keeps its vertex's height
    assert abs(float(P["y_a"]) - ya) < 1e-5 and abs(float(P["y_a"]) - float(seg[0][1])) > 0.05       # interpolated, not the vertex's 0.6
    assert P["rw_a"] > 0 and 1.0 / float(P["rw_a"]) < 0.5 / float(P["rw_b"])                         # (it lies on the near plane, in front of the other end)


# ---- which primitive speaks for the feature ---------------------------------------------------------------

def test_the_primitive_with_the_larger_coverage_speaks_and_the_first_on_a_tie():
    W, H = 96, 64
    h = sc.heights()
    u = uniforms("default", W, H)
    frame, vis = flat(W, H)
    haze = dict(density=0.2, start=1.0)
    eye = np.array([3.0, 2.0, 3.0])
    axis = -eye / np.linalg.norm(eye)
    far, near = (eye + 7.0 * axis).astype(F32), (eye + 3.0 * axis).astype(F32)     # both on the axis: the same screen point, the frame's centre
    recs = np.zeros(2, om.OVIN)
    recs["p0"] = recs["p1"] = [far, near]
    recs["size"] = [1.5, 3.0]                                   # radii: the far disc first, 3 px wide; then the near one, 6 px wide
    recs["flags"] = om.CIRCLE | ohm.HAZE
    recs["rgba"] = 0xFF2010F0
    recs["feature"] = 0
    L = ohm.Layers()
    L.recs.append(recs)
    _, ah, touch = ohm.composite(frame, vis, u, h, GRID, L, haze=haze, want_planes=True)
    probe = lambda k, x, y: ohm.probe(W, H, u, h, GRID, recs[k], x, y, haze)  # noqa: E731
    a_far, a_near = probe(0, 48, 32)["ah"], probe(1, 48, 32)["ah"]
    assert a_far > a_near + 0.3 > 0.3
    assert probe(0, 48, 32)["cover"] == 1.0 == probe(1, 48, 32)["cover"]
    assert bits(ah[32, 48]) == bits(a_far)                       # equal coverage: the first primitive
    assert 0.0 < probe(0, 49, 32)["cover"] < 1.0 == probe(1, 49, 32)["cover"]
    assert bits(ah[32, 49]) == bits(a_near)                      # the far disc's edge: the near one covers more, and speaks
    assert probe(0, 50, 32)["cover"] == 0.0 and bits(ah[32, 50]) == bits(a_near) and touch[32, 50]
    L.recs[0] = recs[::-1].copy()                                 # the other order: the near disc is first and reaches 1 wherever the far one does
    _, ah2, _ = ohm.composite(frame, vis, u, h, GRID, L, haze=haze, want_planes=True)
    assert bits(ah2[32, 48]) == bits(a_near) and bits(ah2[32, 49]) == bits(a_near)


# ---- whole frames ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", sc.CAMS)
def test_the_stencil_and_layers_without_the_flag(cam):
    W, H = 96, 64
    h = sc.heights()
    u = uniforms(cam, W, H)
    frame, vis = flat(W, H, (90, 90, 90, 255))
    haze = sc.settings(cam)["falloff 4.0"]
    calls = sc.layer_calls(cam)
    hazed, plain = layers_of(calls), layers_of(calls, haze=False)
    want_plain = ocm.composite(frame, vis, u, h, GRID, plain)
    out, ah, touch = ohm.composite(frame, vis, u, h, GRID, hazed, haze=haze, want_planes=True)
    assert (out != want_plain).any() and np.array_equal(out[~touch], want_plain[~touch])
    # layers without the flag, and flagged ones without haze or with density 0: the occlusion model's bytes
    assert np.array_equal(ohm.composite(frame, vis, u, h, GRID, plain, haze=haze), want_plain)
    for off in (None, dict(haze, enabled=False), dict(haze, density=0.0)):
        assert np.array_equal(ohm.composite(frame, vis, u, h, GRID, hazed, haze=off), want_plain)
    # a hazed and an unhazed layer interleaved: only the flagged one's pixels move
    mixed = layers_of([(m, a, dict(kw, haze=k % 2 == 0)) for k, (m, a, kw) in enumerate(calls)])
    out_m, _, touch_m = ohm.composite(frame, vis, u, h, GRID, mixed, haze=haze, want_planes=True)
    assert (out_m != want_plain).any() and (out_m != out).any() and np.array_equal(out_m[~touch_m], want_plain[~touch_m])


@pytest.mark.parametrize("size", sc.SIZES)
@pytest.mark.parametrize("cam", sc.CAMS)
def test_the_gpu_files_frames_are_not_vacuous(cam, size):
    """every (camera, size, setting) of tests/test_gpu_overlay_haze.py: at least a quarter of the pixels the hazed layers touch -- counted
    per feature that covers them, as S.ah is per feature -- have 0 < S.ah < max_opacity, and under `fill` and `near` at least one has
    S.ah == 0 (a primitive nearer than `start`)"""
    W, H = size
    h = sc.heights()
    u = uniforms(cam, W, H)
    frame, vis = flat(W, H)
    L = layers_of(sc.layer_calls(cam))
    for name, kw in sc.settings(cam).items():
        _, (n, middle, clear) = ohm.composite(frame, vis, u, h, GRID, L, haze=kw, want_counts=True)
        print(f"{cam} {size} {name}: {n} (hazed feature, pixel) pairs, {middle / n:.2f} with 0 < ah < max_opacity, {clear} with ah == 0")
        assert n > 300 and middle / n >= 0.25, (name, n, middle / n)
        if cam in ("fill", "near"):
            assert clear > 0, name
