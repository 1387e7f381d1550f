"""Feature soak on the GPU box: seeded random scenes through every pass that runs after the tile kernel -- geometry buffers and pick,
the shadow field and the sky-view field, their shade passes, the draped image, point / line / polygon / contour overlays with occlusion
-- on one handle per case, followed by one mutation of the handle (a height upload, a new sun, another image, ...), each step compared with the CPU models
(tests/*_model) run on the oracle's frame.  Every comparison is equality; the one exception is the FAST frame's stated 1 LSB
(include/vf_hip.h).  A sibling of tests/soak_parity.py: test infrastructure, nothing of it is shipped.  A script, and the library of
tests/test_gpu_feature_soak.py (the GPU slice) and tests/test_feature_soak_cases.py (the slice is not vacuous; CPU only).

    case(seed)              a case description: pure numpy and the models' surface sampling, no GPU, no oracle
    CORNERS                 hand-written case descriptions: the edges that must not be left to the draw
    expected(case, state)   the reference frame and planes of a handle state, composed from the models in the library's order:
                            oracle frame -> ambient / shadow shade pass -> draped image -> overlays
    run(first, cases, ...)  the GPU side, case by case

usage: soak_features.py [first_seed] [cases] [time_budget_s]"""
import math, os, sys, time, zlib
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
for _m in ("overlay_model", "polygon_model", "occlusion_model", "contour_model", "gbuffer_model", "shadow_model", "ambient_model", "drape_model"):
    sys.path.insert(0, os.path.join(HERE, _m))
import numpy as np
import ambient_model as abm  # noqa: E402
import contour_model as cm  # noqa: E402
import drape_model as drm  # noqa: E402
import gbuffer_model as gbm  # noqa: E402
import shadow_model as shm  # noqa: E402

ocm = cm.ocm
f32 = np.float32
MUTATIONS = ("heights", "sun", "exaggeration", "clear_overlays", "layer_occlusion", "shadows_off", "reach", "drape_replace", "drape_opacity_zero",
             "drape_clear")
DRAPE_MUTATIONS = MUTATIONS[7:]
GRIDS = (2, 3, 5, 9, 16, 17, 33, 63, 64, 65, 96, 130)
CAPS = ("butt", "square", "round")
SHAPES = ("circle", "square")
JOINS = ("round", "none")
SIZES = (0.3, 1.0, 3.0, 9.0, 30.0, 64.0, 100.0)               # clamped to [1, 64] by the library: the first and the last are
# which fields vf_hip.h says a mutation makes stale (when the field's feature is on)
STALE_SHADOW = ("heights", "sun", "exaggeration")
STALE_AMBIENT = ("heights", "exaggeration", "reach")
# the draped image: widths and heights drawn independently -- one texel, Nx1 and 1xN, texel counts that are and are not
# multiples of k_drape_expand's 256 threads
DRAPE_SIZES = (1, 2, 3, 7, 37, 64, 255, 256, 257, 300)
DRAPE_EXTENTS = ("whole", "interior", "overhanging", "one_side", "off_grid")
DRAPE_FILTERS = ("linear", "nearest")
DRAPE_STREAM = 0xD4A9E                                        # the drape's own generator is default_rng([seed, DRAPE_STREAM])


def _heights(rng, shape, amp, smooth):
    """white noise as test_random_scenes_fuzz draws it, or a few long waves (a surface with slopes that face one way over whole regions)"""
    if not smooth:
        return (rng.random(shape, dtype=f32) - f32(0.5)) * f32(amp)
    X, Z = np.meshgrid(np.linspace(0.0, 1.0, shape[1]), np.linspace(0.0, 1.0, shape[0]))
    h = sum(rng.normal() / f * np.sin(2.0 * math.pi * f * (X * math.cos(a) + Z * math.sin(a)) + p)
            for f, a, p in zip((1, 2, 3), rng.uniform(0, 6.3, 3), rng.uniform(0, 6.3, 3)))
    return (0.25 * amp * h).astype(f32)


def _round(D):
    """the library's default set (include/vf_hip.h: azimuth 360 t / D degrees; whole octants are the exact axes and diagonals), restated
    here so that this module imports without the compiled package"""
    octants = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
    return np.array([octants[8 * t // D] if (8 * t) % D == 0 else (math.cos(2.0 * math.pi * t / D), math.sin(2.0 * math.pi * t / D)) for t in range(D)], f32)


def _directions(rng, kind, D):
    """(D, 2) float32: the default all-round set, a one-sided fan, or an irregular list with axes and exact diagonals"""
    if kind == "round":
        return _round(D)
    if kind == "fan":
        az = rng.uniform(0, 2 * math.pi) + rng.uniform(-0.08, 0.08, D)
        return np.column_stack([np.cos(az), np.sin(az)]).astype(f32)
    special = np.array([(1, 0), (0, -1), (1, 1), (-3, -3), (-1, 1), (0, 2), (1, 1e-3), (-2e-3, 1)], f32)
    az = rng.uniform(0, 2 * math.pi, D)
    d = np.column_stack([np.cos(az), np.sin(az)]).astype(f32) * f32(rng.choice([1.0, 0.01, 50.0]))
    k = min(D, len(special))
    d[rng.permutation(D)[:k]] = special[rng.permutation(len(special))[:k]]
    return d


def _ring(c, radius, k, y, phase=0.0):
    a = phase + 2.0 * math.pi * np.arange(k) / k
    return np.column_stack([c[0] + radius * np.cos(a), np.full(k, y), c[1] + radius * np.sin(a)]).astype(f32)


def _rgba(rng, alpha=None):
    c = [int(v) for v in rng.integers(0, 256, 4)]
    c[3] = int(rng.choice([255, 255, 160, 40])) if alpha is None else alpha
    return tuple(c)


def _overlays(rng, c, surf):
    """The overlay calls of a case, in layer order: (kind, keyword arguments of the model's method).  World x, z span the terrain
    (+-1.5 spacing) and a margin; y is a small offset for draped layers and a world height otherwise."""
    half = 1.6 * c["spacing"]
    yamp = 0.3 * abs(c["exaggeration"]) + 0.05

    def xyz(n, drape):
        return np.column_stack([rng.uniform(-half, half, n), rng.uniform(0.0, 0.05, n) if drape else rng.uniform(-yamp, yamp, n),
                                rng.uniform(-half, half, n)]).astype(f32)

    def occ():
        return dict(occlude=bool(rng.random() < 0.5), depth_bias=float(rng.choice([0.0, 1e-2, 0.2])))

    calls = []
    for shape in SHAPES:                                      # points of both shapes; per-point sizes and colours on one of them
        n = int(rng.integers(1, 40))
        drape = bool(rng.random() < 0.5)
        per = rng.random() < 0.6
        calls.append(("points", dict(xyz=xyz(n, drape), size_px=rng.choice(SIZES, n).astype(f32) if per else float(rng.choice(SIZES)),
                                     rgba=rng.integers(0, 256, (n, 4)).astype(np.uint8) if per else _rgba(rng), shape=shape, drape=drape, **occ())))
    eye, target = np.asarray(c["eye"], np.float64), np.asarray(c["target"], np.float64)
    walk = xyz(1, False)[0] + np.cumsum(rng.normal(0, 0.3 * c["spacing"], (int(rng.integers(2, 7)), 3)) * [1, 0.1, 1], axis=0)
    p, q = xyz(2, False)
    paths = [walk.astype(f32), np.array([p, p, q], f32),                       # a zero-length segment
             np.array([target, eye + 0.7 * (eye - target) + [0.01, 0.02, 0.03]], f32)]   # from the target to behind the eye
    if rng.random() < 0.3:
        paths.append(np.array([q, q], f32))                                    # nothing but a zero-length segment
    order = rng.permutation(3)
    for k, cap in enumerate(CAPS):                            # every cap, the special paths under a different one from case to case
        mine = [paths[order[k]]] + (paths[3:] if k == 0 else [])
        calls.append(("lines", dict(paths=mine, width_px=float(rng.choice([0.5, 1.0, 2.0, 7.0, 80.0])), rgba=_rgba(rng), cap=cap,
                                    drape=bool(rng.random() < 0.3), **occ())))
    ctr = rng.uniform(-0.8, 0.8, 2) * c["spacing"]
    R = float(rng.uniform(0.3, 1.4)) * c["spacing"]
    drape = bool(rng.random() < 0.5)
    y = 0.02 if drape else float(rng.uniform(-yamp, yamp))
    holed = [_ring(ctr, R, int(rng.integers(3, 9)), y), _ring(ctr, 0.5 * R, int(rng.integers(3, 6)), y, 0.4)]
    calls.append(("polygons", dict(polygons=[holed], fill_rgba=_rgba(rng, int(rng.choice([255, 150]))),
                                   line_rgba=_rgba(rng) if rng.random() < 0.5 else None, line_width_px=float(rng.choice([1.0, 3.0])), drape=drape)))
    ctr2 = rng.uniform(-1.2, 1.2, 2) * c["spacing"]
    calls.append(("polygons", dict(polygons=[[_ring(ctr2, 0.6 * R, int(rng.integers(3, 7)), y)]], fill_rgba=None, line_rgba=_rgba(rng),
                                   line_width_px=float(rng.choice([1.0, 2.0, 5.0])), drape=bool(rng.random() < 0.5))))
    fin = surf[np.isfinite(surf)]
    if fin.size:                                              # levels in units of h; one of them a vertex height exactly
        lo, hi = float(fin.min()), float(fin.max())
        lv = np.linspace(lo, hi, int(rng.integers(3, 9)) + 2)[1:-1].astype(f32)
        lv = np.unique(np.concatenate([lv, fin[rng.integers(0, fin.size, 1)]]).astype(f32))
    else:
        lv = np.array([0.0], f32)
    calls.append(("contours", dict(levels=lv, width_px=float(rng.choice([0.5, 1.0, 3.0, 80.0])), rgba=_rgba(rng), lift=float(rng.choice([0.0, 0.02])),
                                   join=str(rng.choice(JOINS)), **occ())))
    return [calls[k] for k in rng.permutation(len(calls))]


def drape_image(rng, iw, ih, channels):
    """(ih, iw, channels) uint8.  RGBA in the pattern of drape_model.image: random colours, alpha 0 in every third cell of 6 x 6 texels
    (of a third of the width or height in an image smaller than 18 texels, so that the linear filter leaves holes in it too) and a
    random value in 1 ... 255 elsewhere -- everywhere, where that would leave no texel to see; RGB: random colours"""
    img = rng.integers(0, 256, (ih, iw, channels), dtype=np.uint8)
    if channels == 4:
        img[..., 3] = rng.integers(1, 256, (ih, iw), dtype=np.uint8)
        cx, cy = max(1, min(6, iw // 3)), max(1, min(6, ih // 3))
        iy, ix = np.meshgrid(np.arange(ih), np.arange(iw), indexing="ij")
        hole = (ix // cx + iy // cy) % 3 == 0
        if not hole.all():
            img[hole, 3] = 0
    return img


def distinct_image(iw, ih):
    """(ih, iw, 4) uint8, opaque, every texel another colour (iw, ih <= 256): a sample names its texel"""
    iy, ix = np.meshgrid(np.arange(ih), np.arange(iw), indexing="ij")
    return np.stack([ix, iy, (ix * 7 + iy * 3) % 256, np.full_like(ix, 255)], axis=2).astype(np.uint8)


def _drape_extent(rng, kind):
    """(x0, z0, x1, z1) in the grid's own plane (vertices at -1.5 ... 1.5, whatever the spacing), or None for the whole grid"""
    def inner():
        a = float(rng.uniform(-1.4, -0.5))
        return a, min(a + float(rng.uniform(1.2, 2.4)), 1.4)

    def over():                                               # beyond the grid at one end, as drape_model.EXTENT is in z
        a, b = inner()
        return (-float(rng.uniform(1.6, 2.5)), b) if rng.random() < 0.5 else (a, float(rng.uniform(1.6, 2.5)))

    if kind == "whole":
        return None
    if kind == "interior":
        (x0, x1), (z0, z1) = inner(), inner()
    elif kind == "overhanging":                               # over a corner of the grid: beyond it in x and in z
        (x0, x1), (z0, z1) = over(), over()
    elif kind == "one_side":
        (x0, x1), (z0, z1) = inner(), inner()
        side = int(rng.integers(0, 4))
        beyond = float(rng.uniform(1.6, 2.5))
        x0, z0, x1, z1 = [(-beyond, z0, x1, z1), (x0, -beyond, x1, z1), (x0, z0, beyond, z1), (x0, z0, x1, beyond)][side]
    else:
        (x0, x1), (z0, z1) = inner(), inner()
        w, off = x1 - x0, float(rng.uniform(1.6, 2.6))
        side = int(rng.integers(0, 4))
        x0, z0, x1, z1 = [(off, z0, off + w, z1), (-off - w, z0, -off, z1), (x0, off, x1, off + w), (x0, -off - w, x1, -off)][side]
    return tuple(float(f32(v)) for v in (x0, z0, x1, z1))


def _drape(rng, must):
    """The drape entry of a case from the drape's own generator: None for about one case in five (never when `must`: the case's
    mutation is one of DRAPE_MUTATIONS), else image, extent, opacity, filter and `replace`, the payload of drape_replace: another
    size, the other channel count, another extent kind and the other filter."""
    absent = rng.random() < 0.2
    iw, ih = (int(v) for v in rng.choice(DRAPE_SIZES, 2))
    channels = int(rng.choice([4, 4, 3]))
    kind = str(rng.choice(DRAPE_EXTENTS, p=[0.06, 0.3, 0.32, 0.27, 0.05]))
    d = dict(image=drape_image(rng, iw, ih, channels), extent=_drape_extent(rng, kind), extent_kind=kind,
             opacity=float(rng.choice([1.0, 0.37, 0.0], p=[0.5, 0.42, 0.08])), filter=str(rng.choice(DRAPE_FILTERS)))
    iw2, ih2 = (int(v) for v in rng.choice(DRAPE_SIZES, 2))
    if (iw2, ih2) == (iw, ih):
        iw2 = DRAPE_SIZES[(DRAPE_SIZES.index(iw) + 1) % len(DRAPE_SIZES)]
    kind2 = str(rng.choice([k for k in DRAPE_EXTENTS if k not in (kind, "off_grid")]))
    d["replace"] = dict(image=drape_image(rng, iw2, ih2, 7 - channels), extent=_drape_extent(rng, kind2), extent_kind=kind2,
                        opacity=float(rng.choice([1.0, 0.37])), filter=DRAPE_FILTERS[1 - DRAPE_FILTERS.index(d["filter"])])
    return None if absent and not must else d


def _make(rng, name, fix, drape_rng, draped=False):
    """A case description; `fix` overrides what the draw would choose (CORNERS).  The drape comes from `drape_rng`, a generator of
    its own: what `rng` gives a seed or a corner does not depend on it; `draped`: never without one (every corner)."""
    c = {"name": name}

    def put(key, draw):
        c[key] = fix[key] if key in fix else draw
        return c[key]

    W, H = put("W", int(rng.integers(1, 400))), put("H", int(rng.integers(1, 300)))
    G = put("grid", int(rng.choice(GRIDS)))
    tex = put("tex", (int(rng.integers(1, 80)), int(rng.integers(1, 80))))
    amp = put("amp", float(rng.choice([0.0, 0.2, 1.0, 3.0])))
    smooth = put("smooth", bool(rng.random() < 0.6))
    h = _heights(rng, tex, amp, smooth)
    if put("nan_texel", bool(rng.integers(0, 4) == 0)):
        h[int(rng.integers(0, tex[0])), int(rng.integers(0, tex[1]))] = np.nan
    put("heights", h)
    r = float(rng.choice([0.05, 0.6, 2.0, 4.5, 9.0]))
    th, ph = rng.uniform(0, 2 * math.pi), rng.uniform(-0.6, 1.4)
    put("eye", (r * math.cos(th) * math.cos(ph), r * math.sin(ph), r * math.sin(th) * math.cos(ph)))
    put("target", tuple(float(v) for v in rng.uniform(-0.4, 0.4, 3)))
    put("fovy", float(rng.choice([20.0, 45.0, 60.0, 120.0, 170.0])))
    put("znear", float(rng.choice([1e-3, 0.1, 0.5 * r])))
    put("zfar", float(rng.choice([r + 0.3, 100.0, 1e4])))     # r + 0.3: the far plane cuts through the terrain
    put("exaggeration", float(rng.choice([1.0, 1.0, 0.0, 8.0, -2.0])))
    put("spacing", float(rng.choice([1.0, 1.0, 0.3, 2.5])))
    special = [(1.0, 0.6, 0.0), (0.0, 0.4, -1.0), (0.5, 0.4, 0.5), (-0.5, 0.3, 0.5), (0.0, 1.0, 0.0), (0.7, 0.0, 0.2), (0.2, -0.3, 0.7)]
    # the sun: of six elevations the one under which the share of shadowed vertices is nearest a quarter, so that the shadows cover
    # part of the surface whatever its relief (the field is the model's: the generator needs no GPU)
    surf = cm.surface(c["heights"], G)
    azimuth, params = rng.uniform(0.0, 360.0), dict(strength=0.7, softness=0.02, bias=0.002)
    share = [float((shm.field_heights(surf, shm.sun_vector(el, azimuth), c["spacing"], c["exaggeration"], **params) < 1).mean()) for el in (5.0, 15.0, 30.0, 50.0, 70.0, 85.0)]
    elevation = (5.0, 15.0, 30.0, 50.0, 70.0, 85.0)[int(np.argmin(np.abs(np.array(share) - 0.25)))]
    sun = shm.sun_vector(elevation, azimuth)
    put("sun", tuple(float(v) for v in (special[int(rng.integers(0, len(special)))] if rng.random() < 0.15 else sun)))
    put("cmap", str(rng.choice(["viridis", "magma", "terrain"])))
    put("mode", int(rng.random() < 0.2))
    mutation = put("mutation", MUTATIONS[int(rng.integers(0, 7))])   # (every caller fixes the mutation; the draw keeps its place in the stream)
    features = put("features", str(rng.choice(["shadows", "ambient", "both"], p=[0.45, 0.3, 0.25])))
    if mutation == "shadows_off" and features == "ambient":
        features = c["features"] = "both"
    if mutation == "reach" and features == "shadows":
        features = c["features"] = "both"
    put("shadows", dict(strength=float(rng.choice([0.7, 1.0, 0.3])), softness=float(rng.choice([0.02, 0.1, 0.5])), bias=float(rng.choice([0.0, 0.002, 0.05]))))
    D = int(rng.choice([1, 2, 3, 4, 8, 16, 33, 64]))
    # every slope is seen from somewhere: an all-round set over any relief leaves no vertex with an open sky (ambient_model.py), so the
    # long waves mostly get a narrow fan that looks one way; with both features on, strength is often 0 (the shadows alone decide
    # what is written again)
    kind = str(rng.choice(["fan", "fan", "fan", "fan", "round", "irregular"] if smooth else ["round", "irregular", "fan"]))
    # (a long reach finds a higher vertex from nearly everywhere: the fans mostly look one or two cells far)
    reach = float(rng.choice([1.0, 1.5, 16.0, 64.0, min(1024.0, math.ceil(1.5 * max(G, 2))), 1024.0], p=[0.3, 0.3, 0.1, 0.1, 0.1, 0.1] if kind == "fan" else None))
    put("ambient", dict(strength=float(rng.choice([0.0, 0.0, 0.6, 1.0] if features == "both" else [0.6, 1.0])), reach=reach, directions=_directions(rng, kind, D)))
    put("overlays", _overlays(rng, c, surf) + list(fix.get("more_overlays", [])))
    # the mutation's payload
    t2 = (int(rng.integers(1, 80)), int(rng.integers(1, 80)))
    if t2 == tuple(c["heights"].shape):
        t2 = (t2[0] + 1, t2[1])
    c["mutation_args"] = dict({
        "heights": _heights(rng, t2, float(rng.choice([0.2, 1.0, 3.0])), bool(rng.random() < 0.5)),
        "sun": tuple(float(v) for v in shm.sun_vector(rng.uniform(5.0, 85.0), rng.uniform(0.0, 360.0))),
        "exaggeration": float(rng.choice([v for v in (0.5, 0.0, 3.0, -1.0) if v != c["exaggeration"]])),
        "layer": int(rng.choice([k for k, (kind_, _) in enumerate(c["overlays"]) if kind_ != "polygons"])),
        "depth_bias": float(rng.choice([0.0, 0.05])),
        "reach": float(rng.choice([v for v in (1.0, 3.0, 40.0, 1024.0) if v != c["ambient"]["reach"]])),
    }, **fix.get("mutation_args", {}))
    # the draped image: drawn whole, then a corner's own fields laid over it (its "replace" replaces the payload whole)
    d = _drape(drape_rng, draped or mutation in DRAPE_MUTATIONS)
    c["drape"] = None if d is None else dict(d, **fix.get("drape", {}))
    return c


def case(seed):
    """The case of a seed: frame, grid, texture, camera and uniforms drawn as test_random_scenes_fuzz draws them, a sun, colormap,
    shade mode, shadow and ambient parameters, which of them are on, the overlay calls, one mutation and (from a generator of its
    own) a draped image or none."""
    return _make(np.random.default_rng(seed), f"seed{seed}", {"mutation": MUTATIONS[seed % len(MUTATIONS)]}, np.random.default_rng([seed, DRAPE_STREAM]))


_CAMERA = dict(eye=(3.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), fovy=45.0, znear=0.1, zfar=100.0)


def _corner(k, name, **fix):
    """the specification of a corner (built by _build when it is first asked for)"""
    return k, name, fix


def _build(k, name, fix):
    """a corner: a well-behaved camera over long waves of amplitude 1, everything on, whatever `fix` does not say drawn from seed k"""
    base = dict(_CAMERA, W=96, H=64, grid=33, tex=(23, 31), amp=1.0, smooth=True, nan_texel=False, exaggeration=1.0, spacing=1.0,
                features="both", mutation=MUTATIONS[k % 7], cmap="viridis", mode=0,     # (the seven mutations older than the drape's: a corner that names none keeps its own)
                shadows=dict(strength=0.7, softness=0.1, bias=0.02))
    base.update(fix)
    if "spacing" in fix and "eye" not in fix:                 # keep the terrain in view
        base["eye"] = tuple(v * fix["spacing"] for v in _CAMERA["eye"])
    return _make(np.random.default_rng(90000 + k), name, base, np.random.default_rng([90000 + k, DRAPE_STREAM]), draped=True)


def _amb(reach, dirs, strength=0.6):
    return dict(strength=strength, reach=float(reach), directions=np.asarray(dirs, f32).reshape(-1, 2))


_FAN = [(-1, 0), (-0.9, 0.31), (-0.9, -0.31)]
_LONG_FOVY = 2.0 * math.degrees(math.atan(0.5 * 1.5 / 6.0))   # from 6 units above, the long side of a frame sees about 0.6 of the terrain's 3 units
# Found by this soak (frame_of_one_column), reduced: a fill whose right edge crosses rows 15-18 at x = 19.4 .. 23.5 of a 17-pixel-wide
# frame -- beyond the frame and inside its last 16-pixel bin column.  k_pg_setup clipped an edge's bins to the frame, the backdrop mask
# gives a bin only the crossings beyond its right edge, so pixel column 16 lost that crossing and the fill
# (tests/test_feature_soak_cases.py asserts where the edge lies).
GAP_RING = np.array([[-0.778, 0.0, -0.354], [0.99, 0.0, -2.121], [2.121, 0.0, -0.99], [0.354, 0.0, 0.778]], f32)
_SPECS = [
    _corner(0, "grid2_frame1x1_sun_up", grid=2, W=1, H=1, sun=(0.0, 1.0, 0.0), tex=(2, 2), ambient=_amb(1.0, _round(4))),
    _corner(1, "grid3_frame15x17_sun_on_horizon", grid=3, W=15, H=17, sun=(0.7, 0.0, 0.2), ambient=_amb(16.0, _FAN)),
    _corner(2, "grid9_frame16x16_sun_below", grid=9, W=16, H=16, sun=(0.2, -0.3, 0.7), ambient=_amb(64.0, _round(16))),
    _corner(3, "grid10_frame17x15_sun_on_axis", grid=10, W=17, H=15, sun=(0.0, 0.4, -1.0), ambient=_amb(3.0, [(0, 1)])),
    _corner(4, "grid63_frame64x64_sun_diagonal", grid=63, W=64, H=64, sun=(-0.5, 0.4, 0.5), ambient=_amb(16.0, [(1, 1), (-1, 1), (1, 0)])),
    _corner(5, "grid64_frame65x63", grid=64, W=65, H=63, smooth=True, ambient=_amb(100.0, _FAN)),
    _corner(6, "grid65_sixty_four_directions", grid=65, W=120, H=70, ambient=_amb(20.0, _round(64))),
    _corner(7, "grid129_one_direction", grid=129, W=150, H=90, smooth=True, ambient=_amb(200.0, [(-0.9, 0.31)])),
    _corner(8, "grid5_reach1", grid=5, ambient=_amb(1.0, _round(8)), mutation="reach", mutation_args={"reach": 1024.0}),
    _corner(9, "grid5_reach1024", grid=5, ambient=_amb(1024.0, _round(8)), mutation="reach", mutation_args={"reach": 1.0}),
    _corner(10, "exaggeration0_spacing0p3", exaggeration=0.0, spacing=0.3, ambient=_amb(16.0, _round(8)),
            mutation="exaggeration", mutation_args={"exaggeration": -2.0}),
    _corner(11, "exaggeration_minus2_spacing2p5", exaggeration=-2.0, spacing=2.5, amp=0.2, ambient=_amb(16.0, _FAN)),
    _corner(12, "texture1x1", tex=(1, 1), ambient=_amb(16.0, _round(8)), mutation="heights"),
    _corner(13, "one_nan_texel", tex=(9, 7), nan_texel=True, ambient=_amb(16.0, _FAN)),
    _corner(14, "all_nan_texture", heights=np.full((5, 6), np.nan, f32), ambient=_amb(16.0, _round(8)), mutation="heights"),
    # the surface is the texture plus an analytic wave of +-0.5: a constant texture of 2^20, where binary32 steps by 1/8, makes it a
    # staircase of plateaus, and the level the draw takes from a vertex lies on a whole plateau (tests/test_gpu_contours.py)
    _corner(15, "constant_texture_level_on_the_plateau", heights=np.full((4, 4), 2.0 ** 20, f32), exaggeration=2.0 ** -20, ambient=_amb(16.0, _round(8)),
            mutation="exaggeration", mutation_args={"exaggeration": 1.5 * 2.0 ** -20}),
    _corner(18, "fill_edge_beyond_the_frame_inside_its_last_bin", W=17, H=33, ambient=_amb(16.0, _FAN),
            more_overlays=[("polygons", dict(polygons=[[GAP_RING]], fill_rgba=(230, 40, 40, 255), line_rgba=None, line_width_px=1.0, drape=False))]),
    _corner(16, "frame_of_one_column", W=1, H=70, grid=17, ambient=_amb(16.0, _FAN)),
    _corner(17, "frame_of_one_row_far_plane_cuts", W=130, H=1, grid=16, zfar=4.8, znear=4.5, ambient=_amb(1.5, _round(3))),
    # the frame limit of the C ABI in either axis: 256 tile columns / rows, 1024 overlay bins, pixel boxes at the end of int16.  A camera
    # looking steeply down (up stays +y, so x runs along the width and z down the height) whose narrow field of view lets the terrain
    # overfill the long side; a line on the world axis that projects to the frame's centre row / column carries an overlay into the last bin (tests/test_feature_soak_cases.py asserts it)
    _corner(19, "frame16384x24", W=16384, H=24, grid=257, eye=(0.0, 6.0, 0.6), fovy=_LONG_FOVY / (16384 / 24), znear=0.1, zfar=100.0, ambient=_amb(8.0, _FAN),
            more_overlays=[("lines", dict(paths=[np.array([[-1.6, 0.0, 0.0], [1.6, 0.0, 0.0]], f32)], width_px=3.0, rgba=(250, 220, 30, 255), cap="butt",
                                          drape=False, occlude=False, depth_bias=0.0))]),
    _corner(20, "frame24x16384", W=24, H=16384, grid=257, eye=(0.0, 6.0, 0.6), fovy=_LONG_FOVY, znear=0.1, zfar=100.0, ambient=_amb(16.0, _FAN),
            more_overlays=[("lines", dict(paths=[np.array([[0.0, 0.0, -1.6], [0.0, 0.0, 1.6]], f32)], width_px=3.0, rgba=(250, 220, 30, 255), cap="butt",
                                          drape=False, occlude=False, depth_bias=0.0))]),
    # the draped image's own edges (tests/test_feature_soak_cases.py asserts what each is named for)
    # one texel under the linear filter: all four taps clamp to it; a border pixel whose interpolated x rounds beyond +-1.5 is not written
    _corner(21, "drape_1x1_linear_full_extent", mutation="drape_opacity_zero", ambient=_amb(16.0, _FAN, strength=0.0),
            drape=dict(image=np.array([[(200, 90, 33, 180)]], np.uint8), extent=None, extent_kind="whole", opacity=1.0, filter="linear")),
    # x1 - x0 is inf in binary32 and sx = 0: every covered pixel takes texel (0, 0)
    _corner(22, "drape_extent_overflows", mutation="drape_replace", ambient=_amb(16.0, _FAN),
            drape=dict(image=distinct_image(7, 5), extent=(-3e38, -3e38, 3e38, 3e38), extent_kind="overflows", opacity=1.0, filter="linear")),
    _corner(23, "drape_extent_off_the_grid", mutation="heights", ambient=_amb(16.0, _FAN),
            drape=dict(image=distinct_image(37, 64), extent=(1.6, -1.0, 2.9, 1.0), extent_kind="off_grid", opacity=1.0, filter="linear")),
    _corner(24, "drape_transparent_image", mutation="drape_replace", ambient=_amb(16.0, _FAN),
            drape=dict(image=distinct_image(37, 7) * np.array([1, 1, 1, 0], np.uint8), extent=None, extent_kind="whole", opacity=1.0, filter="linear",
                       replace=dict(image=distinct_image(64, 3)[..., :3].copy(), extent=None, extent_kind="whole", opacity=1.0, filter="nearest"))),
    # the eye low over the middle of a coarse grid: the near plane cuts triangles the image covers, so k_relight<true, kDrape> sends lit
    # and amb through the clipper in the place of the height, under a low sun and an ambient fan that leave neither at 1;
    # then the shadows go while the drape stays
    _corner(25, "drape_near_plane_through_the_terrain", grid=9, eye=(0.9, 0.7, 0.8), target=(-0.4, -0.2, -0.3), znear=0.4, fovy=60.0,
            sun=tuple(float(v) for v in shm.sun_vector(15.0, 200.0)), shadows=dict(strength=0.7, softness=0.1, bias=0.02),
            ambient=_amb(16.0, _FAN, strength=0.6), mutation="shadows_off",
            drape=dict(image=distinct_image(37, 64), extent=(-0.9, -1.0, 0.6, 0.7), extent_kind="interior", opacity=0.37, filter="linear")),
    # the extent lies in the grid's own plane, whatever the spacing: an interior box, the nearest filter, every texel distinct
    _corner(26, "drape_under_spacing_2p5_exaggeration_minus2", spacing=2.5, exaggeration=-2.0, amp=0.2, mutation="exaggeration", ambient=_amb(16.0, _FAN, strength=0.0),
            drape=dict(image=distinct_image(37, 64), extent=(-0.7, -0.5, 0.9, 0.8), extent_kind="interior", opacity=1.0, filter="nearest")),
    _corner(27, "drape_under_spacing_0p3", spacing=0.3, exaggeration=0.3, eye=(0.5, 0.9, 0.5), mutation="sun", ambient=_amb(16.0, _FAN),
            drape=dict(image=distinct_image(64, 37), extent=(-0.7, -0.5, 0.9, 0.8), extent_kind="interior", opacity=1.0, filter="nearest")),
    _corner(28, "drape_denser_than_the_frame", W=15, H=17, mutation="drape_clear", ambient=_amb(16.0, _FAN),
            drape=dict(image=drape_image(np.random.default_rng(28), 300, 300, 4), extent=None, extent_kind="whole", opacity=1.0, filter="linear")),
]


class _Corners:
    """CORNERS: a sequence of case descriptions.  The names are known at import; a case is made when it is first asked for (the
    generator samples the surface and scans the shadow field six times: a collection that runs none of them pays for none)."""

    def __init__(self, specs):
        self._specs, self._made = specs, {}
        self.names = [name for _, name, _ in specs]

    def __len__(self):
        return len(self._specs)

    def __getitem__(self, i):
        if i not in self._made:
            self._made[i] = _build(*self._specs[range(len(self._specs))[i]])
        return self._made[i]

    def __iter__(self):
        return (self[i] for i in range(len(self._specs)))

    def named(self, name):
        return self[self.names.index(name)]


CORNERS = _Corners(_SPECS)


# ---- the reference ---------------------------------------------------------------------------------------------------

_luts = None


def lut(name):
    global _luts
    if _luts is None:
        _luts = np.load(os.path.join(HERE, "golden", "colormaps_rgba8.npz"))
    return _luts[name]


def uniforms(c, sun=None, exaggeration=None):
    """the uniform block of a case (oracle.look_at_uniforms raises for a degenerate camera)"""
    import oracle
    u = np.array(oracle.look_at_uniforms(1, c["W"], c["H"], c["eye"], c["target"], (0.0, 1.0, 0.0), c["fovy"], c["znear"], c["zfar"]), f32).reshape(44)
    u[38] = c["exaggeration"] if exaggeration is None else exaggeration
    u[36] = c["spacing"]
    u[32:35] = c["sun"] if sun is None else sun
    return u


def initial_state(c):
    """the handle's state before any feature is on: what `expected` and `run` step through"""
    return dict(heights=c["heights"], u=uniforms(c), shadows=False, ambient=False, shadow_params=dict(c["shadows"]), ambient_params=dict(c["ambient"]),
                overlays=False, occlusion={}, drape=None)


def the_drape(d):
    """what a handle state holds of a drape entry: the arguments of set_drape"""
    return None if d is None else {k: d[k] for k in ("image", "extent", "opacity", "filter")}


def featured(c, state, overlays=False, drape=True):
    """the state with the case's shade features on and, unless `drape` is false, its draped image set"""
    return dict(state, shadows=c["features"] in ("shadows", "both"), ambient=c["features"] in ("ambient", "both"), overlays=overlays,
                drape=the_drape(c["drape"]) if drape else state["drape"])


def mutated(c, state):
    """the state after the case's mutation"""
    kind, a = c["mutation"], c["mutation_args"]
    s = dict(state)
    if kind == "heights":
        s["heights"] = a["heights"]
    elif kind == "sun":
        s["u"] = uniforms(c, sun=a["sun"], exaggeration=state["u"][38])
    elif kind == "exaggeration":
        s["u"] = uniforms(c, sun=state["u"][32:35], exaggeration=a["exaggeration"])
    elif kind == "clear_overlays":
        s["overlays"], s["occlusion"] = False, {}
    elif kind == "layer_occlusion":
        k = a["layer"]
        s["occlusion"] = {**state["occlusion"], k: (not c["overlays"][k][1]["occlude"], a["depth_bias"])}
    elif kind == "shadows_off":
        s["shadows"] = False
    elif kind == "reach":
        s["ambient_params"] = dict(state["ambient_params"], reach=a["reach"])
    elif kind == "drape_replace":
        s["drape"] = the_drape(c["drape"]["replace"])
    elif kind == "drape_opacity_zero":                        # (the same image set again; on a handle without one, the case's)
        s["drape"] = dict(state["drape"] or the_drape(c["drape"]), opacity=0.0)
    elif kind == "drape_clear":
        s["drape"] = None
    return s


def layers(c, state):
    """The models' layers of the case's overlay calls.  The snapshot rule of vf_terrain_add_contours (include/vf_hip.h): a contour layer
    is made from the heights and the spacing the handle held when it was added -- the case's own, every mutation comes later -- so a
    later height upload does not move its records; they are draped, so the composite, which gets the state's heights and uniforms,
    follows a later exaggeration."""
    L = cm.Layers()
    L.segments = {}                                           # call index -> segments of a contour layer
    u0 = uniforms(c)
    index = {}                                                # layer id of the library -> index among the models' point / line layers
    for k, (kind, kw) in enumerate(c["overlays"]):
        if kind == "points":
            L.points(kw["xyz"], **{a: v for a, v in kw.items() if a != "xyz"})
        elif kind == "lines":
            L.lines(kw["paths"], **{a: v for a, v in kw.items() if a != "paths"})
        elif kind == "polygons":
            L.polygons(kw["polygons"], **{a: v for a, v in kw.items() if a != "polygons"})
            continue
        else:
            L.contours(c["heights"], c["grid"], u0, kw["levels"], **{a: v for a, v in kw.items() if a != "levels"})
            L.segments[k] = L.nsegments
        index[k] = len(L.ranges) - 1
    L.counts = {}
    for k, (kind, kw) in enumerate(c["overlays"]):
        if kind != "polygons":
            a, b = L.ranges[index[k]]
            L.counts[k] = sum(len(r) for r in L.recs[a:b])
    for k, (occlude, bias) in state["occlusion"].items():
        L.set_occlusion(index[k], occlude, bias)
    return L


def expected(c, state, cache=None):
    """The reference of a handle state, in the order the library documents: the oracle's frame and visibility; the shade pass
    (ambient_model.frame with the shadow field when both are on, shadow_model.frame for shadows alone); the overlays
    the draped image over that frame (drape_model.frame, with the state's shadow and sky-view fields and strength when those
    features are on); the overlays (occlusion_model.composite of the contour model's layers).  `cache` (a dict of one case) keeps
    the oracle's frames and the results, for a caller that asks for a state twice.  -> dict rgba (the oracle's frame), vis, shaded,
    mask (the pixels the shade pass writes again), draped (the frame behind the drape pass: `shaded` without a drape), drape_mask
    (the pixels the drape writes again), frame (what the handle must show), layers (or None)."""
    import oracle
    W, H, G, h, u = c["W"], c["H"], c["grid"], state["heights"], state["u"]
    key = (u.tobytes(), h.tobytes(), h.shape)
    A, D = state["ambient_params"], state["drape"]
    whole = (key, state["shadows"], state["ambient"], state["overlays"], tuple(sorted(state["shadow_params"].items())),
             A["strength"], A["reach"], A["directions"].tobytes(), tuple(sorted(state["occlusion"].items())),
             None if D is None else (D["image"].tobytes(), D["image"].shape, D["extent"], D["opacity"], D["filter"]))
    if cache is not None and whole in cache:
        return cache[whole]
    if cache is not None and key in cache:
        rgba, vis = cache[key]
    else:
        rgba, vis = oracle.render_terrain(u, W, H, G, h, lut(c["cmap"]), want_vis=True, nthreads=min(8, oracle.max_threads()), shade_mode=c["mode"])
        rgba = rgba.reshape(H, W, 4)
        if cache is not None:
            cache[key] = (rgba, vis)
    out = {"rgba": rgba, "vis": vis, "shaded": rgba, "mask": np.zeros((H, W), bool), "layers": None}
    shade = ("shade",) + whole[:3] + whole[4:8]               # the fields and the shade pass: the same under any drape and any overlays
    if cache is not None and shade in cache:
        lit, sky, out["shaded"], out["mask"] = cache[shade]
    else:
        lit = shm.field(u, h, G, **state["shadow_params"]) if state["shadows"] else None
        sky = None
        if state["ambient"]:
            sky = abm.field(u, h, G, A["directions"], A["reach"])
            out["shaded"], out["mask"] = abm.frame(rgba, vis, u, h, G, lut(c["cmap"]), sky, A["strength"], lit=lit, shade_mode=c["mode"])
        elif state["shadows"]:
            out["shaded"], out["mask"] = shm.frame(rgba, vis, u, h, G, lut(c["cmap"]), lit, shade_mode=c["mode"])
        if cache is not None:
            cache[shade] = (lit, sky, out["shaded"], out["mask"])
    out["draped"], out["drape_mask"] = out["shaded"], np.zeros((H, W), bool)
    if D is not None:
        out["draped"], out["drape_mask"] = drm.frame(out["shaded"], vis, u, h, G, lut(c["cmap"]), D["image"], extent=D["extent"], opacity=D["opacity"],
                                                     filter=D["filter"], lit=lit, sky=sky, strength=A["strength"],
                                                     shade_mode=c["mode"])
    out["frame"] = out["draped"]
    if state["overlays"]:
        out["layers"] = layers(c, state)
        out["frame"] = ocm.composite(out["draped"], vis, u, h, G, out["layers"])
    if cache is not None:
        cache[whole] = out
    return out


def planes(c, state, vis):
    depth, position, normal = gbm.planes(vis, state["u"], state["heights"], c["grid"])
    return {"depth": depth, "position": position, "normal": normal, "primitive": vis}


def shares(c, cache=None):
    """what the reference alone says about a case (tests/test_feature_soak_cases.py): the share of covered pixels, the share of the
    covered pixels the shade pass writes again, the share the drape writes again (None without a drape or without a covered pixel),
    whether the drape's pixels and the shade pass's overlap with each having pixels the other lacks, whether the overlays change a
    pixel"""
    s0 = initial_state(c)
    e = expected(c, featured(c, s0, overlays=True), cache)
    covered = int((e["vis"] != 0).sum())
    m, d = e["mask"], e["drape_mask"]
    return dict(covered=covered / e["vis"].size, rewritten=(int(m.sum()) / covered) if covered else None,
                draped=(int(d.sum()) / covered) if covered and c["drape"] is not None else None,
                masks_cross=bool((m & d).any() and (m & ~d).any() and (d & ~m).any()),
                overlays_show=bool((e["frame"] != e["draped"]).any()))


# ---- the GPU side ----------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _where(d):
    return int(d.sum()), np.argwhere(d)[:4].tolist()


def _add_overlays(t, c):
    """the case's overlay calls on the handle -> (layer ids, contour segment counts by call index)"""
    ids, nseg = {}, {}
    for k, (kind, kw) in enumerate(c["overlays"]):
        if kind == "points":
            ids[k] = t.add_points(kw["xyz"], size_px=kw["size_px"], rgba=kw["rgba"], shape=SHAPES.index(kw["shape"]), drape=kw["drape"])
        elif kind == "lines":
            offs = np.concatenate([[0], np.cumsum([len(p) for p in kw["paths"]])]).astype(np.uint32)
            ids[k] = t.add_lines(np.concatenate(kw["paths"]), offs, width_px=kw["width_px"], rgba=kw["rgba"], cap=CAPS.index(kw["cap"]), drape=kw["drape"])
        elif kind == "polygons":
            rings = [r for poly in kw["polygons"] for r in poly]
            roffs = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.uint32)
            foffs = np.concatenate([[0], np.cumsum([len(poly) for poly in kw["polygons"]])]).astype(np.uint32)
            ids[k] = t.add_polygons(np.concatenate(rings), roffs, foffs, fill_rgba=kw["fill_rgba"], line_rgba=kw["line_rgba"],
                                    line_width_px=kw["line_width_px"], drape=kw["drape"])
        else:
            ids[k], nseg[k] = t.add_contours(kw["levels"], width_px=kw["width_px"], rgba=kw["rgba"], lift=kw["lift"], join=JOINS.index(kw["join"]),
                                             occlude=kw["occlude"], depth_bias=kw["depth_bias"])
        if kind in ("points", "lines") and kw["occlude"]:
            t.set_layer_occlusion(ids[k], True, kw["depth_bias"])
        assert ids[k] == k
    return ids, nseg


def _set_features(t, state):
    P = state["ambient_params"]
    t.set_shadows(state["shadows"], **state["shadow_params"])
    t.set_ambient_occlusion(state["ambient"], strength=P["strength"], reach=P["reach"], directions=P["directions"])


def _set_drape(t, D):
    """the state's drape on the handle -> what drape_info() must say then"""
    if D is None:
        t.clear_drape()
        return None
    t.set_drape(D["image"], extent=D["extent"], opacity=D["opacity"], filter=D["filter"])
    ih, iw = D["image"].shape[:2]
    return dict(width=iw, height=ih, extent=tuple(float(f32(v)) for v in (drm.FULL_EXTENT if D["extent"] is None else D["extent"])),
                opacity=float(f32(D["opacity"])), filter=D["filter"])


def run_case(c, seed=None, cache=None):
    """One case on one handle -> list of (seed, step, what, count of differing pixels or vertices, first four positions)."""
    from vulkan_forge_amd import cabi
    seed = c["name"] if seed is None else seed
    bad, cache = [], {} if cache is None else cache
    W, H, G = c["W"], c["H"], c["grid"]

    def differ(step, what, d):
        if d.any():
            bad.append((seed, step, what) + _where(d))

    def frame(t):
        t.render()
        return t.read_rgba().reshape(H, W, 4)

    def compare_planes(step, state, vis):
        want = planes(c, state, vis)
        got = t.read_gbuffer()
        for k in want:
            differ(step, f"gbuffer {k}", _bits(got[k]) != _bits(want[k]))
        return want

    state = initial_state(c)
    t = cabi.Terrain(W, H, G, lut(c["cmap"]))
    try:
        # 1. exact precision, nothing enabled: the frame, the visibility, the planes, pick
        t.set_uniforms(state["u"]); t.set_shade_mode(c["mode"]); t.set_height(state["heights"]); t.set_shade_precision(0)
        e = expected(c, state, cache)
        differ(1, "frame", (frame(t) != e["frame"]).any(axis=2))
        differ(1, "visibility", t.read_visibility() != e["vis"])
        want = compare_planes(1, state, e["vis"])
        rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
        px = np.concatenate([[[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.column_stack([rng.integers(0, W, 12), rng.integers(0, H, 12)])]).astype(np.int32)
        got, ref = t.pick(px), gbm.pick(px, e["vis"], state["u"], state["heights"], G)
        for k in ref:
            differ(1, f"pick {k}", (_bits(got[k]) != _bits(ref[k])).reshape(len(px), -1).any(axis=1))
            differ(1, f"pick {k} against the planes", (_bits(ref[k]) != _bits(want[k][px[:, 1], px[:, 0]])).reshape(len(px), -1).any(axis=1))
        # 2. the fields and the height bounds
        _set_features(t, state)                               # (off: the parameters alone)
        differ(2, "shadow field", _bits(t.shadow_field()) != _bits(shm.field(state["u"], state["heights"], G, **state["shadow_params"])))
        P = state["ambient_params"]
        differ(2, "sky-view field", _bits(t.sky_view_field()) != _bits(abm.field(state["u"], state["heights"], G, P["directions"], P["reach"])))
        lo_hi, ref_lo_hi = t.height_bounds(), cm.bounds(cm.surface(state["heights"], G))
        if lo_hi != ref_lo_hi:
            bad.append((seed, 2, f"height bounds {lo_hi} against {ref_lo_hi}", 1, []))
        # 3. fast precision, the shade features on, no overlays
        t.set_shade_precision(1)
        plain = frame(t).copy()
        differ(3, "fast frame more than 1 LSB from the oracle", (np.abs(plain.astype(np.int16) - e["rgba"].astype(np.int16)) > 1).any(axis=2))
        state = featured(c, state, drape=False)
        _set_features(t, state)
        e = expected(c, state, cache)
        got = frame(t)
        differ(3, "rewritten pixels", (got != e["shaded"]).any(axis=2) & e["mask"])
        differ(3, "other pixels against the frame before", (got != plain).any(axis=2) & ~e["mask"])
        differ(3, "other pixels more than 1 LSB from the oracle", (np.abs(got.astype(np.int16) - e["rgba"].astype(np.int16)) > 1).any(axis=2) & ~e["mask"])
        if t.drape_info() is not None:
            bad.append((seed, 3, "drape_info() of a handle that never had a drape is not None", 1, []))
        if c["drape"] is not None:                            # the draped image, still in fast precision; the second frame is the one planned ahead
            state = featured(c, state)
            info = _set_drape(t, state["drape"])
            if t.drape_info() != info:
                bad.append((seed, 3, f"drape_info() {t.drape_info()} against {info}", 1, []))
            e = expected(c, state, cache)
            for again in ("", " drawn again"):
                got = frame(t)
                differ(3, "draped pixels" + again, (got != e["draped"]).any(axis=2) & e["drape_mask"])
                differ(3, "rewritten pixels outside the drape" + again, (got != e["shaded"]).any(axis=2) & e["mask"] & ~e["drape_mask"])
                differ(3, "other pixels against the frame before" + again, (got != plain).any(axis=2) & ~e["mask"] & ~e["drape_mask"])
        # 4. exact precision, the overlays
        t.set_shade_precision(0)
        ids, nseg = _add_overlays(t, c)
        state = dict(state, overlays=True)
        e = expected(c, state, cache)
        L = e["layers"]
        for k in nseg:
            if nseg[k] != L.segments[k]:
                bad.append((seed, 4, f"contour layer {k}: {nseg[k]} segments against {L.segments[k]}", 1, []))
        for k in L.counts:
            n = t.layer_primitive_count(ids[k])
            if n != L.counts[k]:
                bad.append((seed, 4, f"layer {k}: {n} primitives against {L.counts[k]}", 1, []))
        differ(4, "frame", (frame(t) != e["frame"]).any(axis=2))
        differ(4, "frame drawn again", (frame(t) != e["frame"]).any(axis=2))
        compare_planes(4, state, e["vis"])                    # (the planes and the visibility know nothing of the drape)
        differ(4, "visibility", t.read_visibility() != e["vis"])
        # 5. the mutation
        kind, a = c["mutation"], c["mutation_args"]
        scans = (t.shadow_scans(), t.ambient_scans())
        state = mutated(c, state)
        if kind == "heights":
            t.set_height(state["heights"])
        elif kind in ("sun", "exaggeration"):
            t.set_uniforms(state["u"])
        elif kind == "clear_overlays":
            t.clear_overlays()
        elif kind == "layer_occlusion":
            t.set_layer_occlusion(ids[a["layer"]], *state["occlusion"][a["layer"]])
        elif kind in DRAPE_MUTATIONS:
            info = _set_drape(t, state["drape"])
            if t.drape_info() != info:
                bad.append((seed, 5, f"drape_info() {t.drape_info()} against {info} after {kind}", 1, []))
        else:
            _set_features(t, state)
        e = expected(c, state, cache)
        differ(5, f"frame after {kind}", (frame(t) != e["frame"]).any(axis=2))
        if kind == "drape_opacity_zero":                      # nothing is written by the drape: the frame of the state without one
            differ(5, "frame at opacity 0 against the state without a drape", (frame(t) != expected(c, dict(state, drape=None), cache)["frame"]).any(axis=2))
        rose = (t.shadow_scans() - scans[0], t.ambient_scans() - scans[1])
        must = (int(state["shadows"] and kind in STALE_SHADOW), int(state["ambient"] and kind in STALE_AMBIENT))
        if rose != must:
            bad.append((seed, 5, f"after {kind} the shadow / sky-view field was computed {rose} times, the contract says {must}", 1, []))
        # 6. the drape cleared: the frame of the same state without one
        if state["drape"] is not None:
            state = dict(state, drape=None)
            _set_drape(t, None)
            differ(6, "frame after clear_drape", (frame(t) != expected(c, state, cache)["frame"]).any(axis=2))
        if t.drape_info() is not None:
            bad.append((seed, 6, f"drape_info() {t.drape_info()} after clear_drape", 1, []))
    finally:
        t.close()
    return bad


FRESH_SEED = 50000                                            # the script's default window: apart from the suite's (test_gpu_feature_soak.py)
MAX_SKIPPED = 0.1                                             # the share of the seeds that may be skipped for a degenerate camera


def run(first=FRESH_SEED, cases=200, budget=400.0, verbose=True, corners=True):
    """CORNERS first (unless `corners` is false: the suite runs them as tests of their own), then seeds first .. first + cases - 1
    (until `budget` seconds have passed) -> dict: cases (seeds done), corners (done), skipped (seeds with a degenerate camera), bad
    (the tuples of run_case), summary."""
    t0 = time.time()
    say = (lambda *a: print(*a, flush=True)) if verbose else (lambda *a: None)
    bad, done, skipped, stat = [], 0, 0, []

    def one(c, seed):
        cache = {}
        stat.append(shares(c, cache))
        b = run_case(c, seed, cache)
        for m in b:
            say(f"MISMATCH {m[0]} step {m[1]}: {m[2]}: {m[3]} differ, first at {m[4]}  ({c['W']}x{c['H']} grid={c['grid']} {c['features']} mutation={c['mutation']})")
        bad.extend(b)

    ncorners = 0
    for c in (CORNERS if corners else ()):
        one(c, None)
        ncorners += 1
    if corners:
        say(f"{ncorners} corners, {len(bad)} mismatches, {time.time() - t0:.0f} s")
    for seed in range(first, first + cases):
        if time.time() - t0 > budget:
            break
        c = case(seed)
        try:
            uniforms(c)
        except RuntimeError:
            skipped += 1                                      # a degenerate camera (the view direction parallel to up, ...): nothing else is caught
            continue
        one(c, seed)
        done += 1
        if done % 25 == 0:
            say(f"{done} cases, {len(bad)} mismatches, {time.time() - t0:.0f} s")
    share = skipped / max(done + skipped, 1)
    summary = (f"feature soak: {ncorners} corners and {done} cases from seed {first}, {skipped} skipped for a degenerate camera ({100.0 * share:.0f} %, "
               f"bound {100.0 * MAX_SKIPPED:.0f} %): {len(bad)} mismatches; {describe(stat)}; {time.time() - t0:.0f} s")
    say(summary)
    return {"cases": done, "corners": ncorners, "skipped": skipped, "too_many_skipped": share > MAX_SKIPPED, "bad": bad, "summary": summary}


def describe(stat):
    """the shares of tests/test_feature_soak_cases.py over a list of shares() results, as text"""
    n = max(len(stat), 1)
    shaded = [s["rewritten"] for s in stat if s["rewritten"] is not None]
    partial = sum(0.1 < r < 0.9 for r in shaded)
    draped = [s for s in stat if s["draped"] is not None]
    return (f"{100.0 * sum(s['covered'] > 0.05 for s in stat) / n:.0f} % of the cases with more than 5 % of the pixels covered, "
            f"{100.0 * partial / max(len(shaded), 1):.0f} % of the covered ones rewrite 10-90 % of the covered pixels, "
            f"{len(draped)} draped and covered cases of which the drape rewrites 10-90 % of the covered pixels in "
            f"{100.0 * sum(0.1 < s['draped'] < 0.9 for s in draped) / max(len(draped), 1):.0f} % and crosses the shade pass's pixels in "
            f"{100.0 * sum(s['masks_cross'] for s in draped) / max(len(draped), 1):.0f} %, "
            f"overlays change a pixel in {100.0 * sum(s['overlays_show'] for s in stat) / n:.0f} %")


if __name__ == "__main__":
    first = int(sys.argv[1]) if len(sys.argv) > 1 else FRESH_SEED
    cases = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    budget = float(sys.argv[3]) if len(sys.argv) > 3 else 400.0
    res = run(first, cases, budget)
    sys.exit(1 if res["bad"] or res["too_many_skipped"] else 0)
