"""Feature soak on the GPU box: seeded random scenes through every pass that runs after the tile kernel -- geometry buffers and pick,
the shadow field and the sky-view field, their shade passes, the draped image, point / line / polygon / contour overlays with occlusion,
of which the point, line and contour layers may take the haze -- on one handle per case, followed by one mutation of the handle (a height upload, a new sun, another image, ...), each step compared with the CPU models
(tests/*_model) run on the oracle's frame.  Every comparison is equality; the one exception is the FAST frame's stated 1 LSB
(include/vf_hip.h).  A sibling of tests/soak_parity.py: test infrastructure, nothing of it is shipped.  A script, and the library of
tests/test_gpu_feature_soak.py (the GPU slice) and tests/test_feature_soak_cases.py (the slice is not vacuous; CPU only).

    case(seed)              a case description: pure numpy and the models' surface sampling, no GPU, no oracle
    CORNERS                 hand-written case descriptions: the edges that must not be left to the draw
    expected(case, state)   the reference frame and planes of a handle state: the oracle's frame, the passes in the library's order,
                            which supersample_model.chain alone writes down, then the overlays under the state's haze
                            (overlay_haze_model.composite: the soak has no arithmetic of its own)
    run(first, cases, ...)  the GPU side, case by case

The late passes ride on the same handle, between the overlays and the mutation: the drape's mip pyramid and
anisotropic taps, the viewshed, cumulative-viewshed and sun-exposure fields and tints, the haze; then a second mutation of their own,
and for a case with a factor above 1 a supersampled second handle.  The flood and the spill (the two passes between
the drape and the exposure tint, whose fields iterate to a fixpoint across launches) ride with them, and get a third mutation of
their own.  Hazed overlay layers ride on the overlays: a case's `hazed` entry says which of its point, line and contour
layers are flagged and whether directly after their add or after all adds, and puts a ladder of twelve hazed draped circles from under
the eye through the target behind them; step 4 sets the flags while the haze is still off (the unflagged bytes, layer_haze() of every
layer), every later frame is compared under the flags, and a fourth mutation (flag_flip, flags_all_off, haze_params,
occlusion_on_hazed, readd, polygon_refused) comes in a step of its own.  Steps A - E, H and W of run_case:
    A  the three vertex fields, bit for bit, their passes off; the cumulative and exposure fields again at another batch size; the
       flood, spill and sink-depth fields with flood_info() and spill_info() (counts, mode, seeds' vertices, passes and tile runs
       inside the bounds of the models' tile_passes), and again at another group size, the spill's with or without its activity flags
    B  the passes on in exact precision: the frame (twice), the haze opacity plane, drape_mip_info() and one pyramid level
    C  fast precision.  The handle exposes no frame from between its passes, and needs none: the relight and drape passes write the
       same bytes in either precision (step 3 found that without mips; with the mips and the anisotropic taps on it is asserted here,
       not derived from step 3), and every other pixel is the plain fast frame's, so the fast frame before the late passes is known,
       and the tints and the haze, which do not follow the precision, must give their models' bytes over it -- on written pixels and
       others alike.  The pixels an overlay touches are left out of the colour comparison altogether, the 1 LSB bound included (the
       overlays blend over bytes that may be 1 LSB off, and where a layer is opaque nothing of the frame beneath is left to compare);
       the alpha channel is compared everywhere
    H  the hazed mutation, while everything is on: the frame, layer_haze() of every layer; for readd clear_overlays with flags set,
       layer_haze refused for the old ids, every call added again unflagged, then again with the flags set the other way round
       (early <-> late); for polygon_refused the two messages and an unchanged frame
    D  the mutation (step 5) and the late mutation: the frame, and the rise of the five scan counters and of the pyramid's builds
       against STALE_VIEWSHED, STALE_CUMULATIVE, STALE_EXPOSURE, STALE_FLOOD, STALE_SPILL and MIP_BUILDS
    W  the water mutation: the frame (for spill_cleared: the frame without the spill, then with it set again) and the same counters
    E  supersample=f: the samples, the resolved frame under the overlays (none occluding; the flags and the ladder as on the first
       handle) and the samples' visibility, again after the late mutation and after the water mutation

usage: soak_features.py [first_seed] [cases] [time_budget_s]"""
import hashlib, math, os, sys, time, zlib
import numpy as np
import model_support  # noqa: F401  (first: the repository root and the model directories on sys.path)
import ambient_model as abm
import contour_model as cm
import cumulative_viewshed_model as cvm
import drape_mip_model as dmm
import drape_model as drm
import flood_model as fdm
import gbuffer_model as gbm
import haze_model as hzm
import occlusion_model as ocm
import overlay_haze_model as ohm
import shadow_model as shm
import spill_model as spm
import sun_exposure_model as sem
import supersample_model as ssm
import viewshed_model as vsm

HERE = os.path.dirname(os.path.abspath(__file__))
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
# the late passes: the drape's mips and anisotropy, the three tints with their vertex fields, haze, supersampling.
# Their generator is default_rng([seed, LATE_STREAM]): no key a case had before them depends on it (OLD_KEYS, digest)
LATE_STREAM = 0x1A7E
LATE_PASSES = ("mips", "viewshed", "cumulative", "exposure", "haze")
LATE_MUTATIONS = ("observer_moves", "observer_same_vertex", "radius", "cumulative_reorder", "suns_reweight", "incidence_flip", "haze_off", "mips_off",
                  "mips_bias", "anisotropy", "tint_colours_only", "heights_again")
MIP_MUTATIONS = ("mips_off", "mips_bias", "anisotropy")
MIP_BIASES = (0.0, -1.0, 1.5, 16.0, -16.0)
ANISOTROPIES = (1, 2, 4, 8, 16)
FACTORS = (1, 1, 2, 3, 4)
OBSERVER_COUNTS = (1, 2, 7, 33)
SUN_COUNTS = (1, 3, 12)
OBSERVER_BATCHES = (0, 1, 3)
SUN_BATCHES = (0, 1, 2)
SOFTNESS = (1e-6, 0.02, 0.5)                                  # (the C ABI refuses a softness of 0: the hard edge is the smallest step that it takes)
SAMPLE_CAP = 1 << 20                                          # f f W H above this: f = 1 (a bound on the cost of the CPU models, not a measurement)
# which vertex fields vf_hip.h says a mutation (of either kind) makes stale, when the field's tint is on: the viewshed's after the
# heights, the exaggeration, the observer's vertex or a scan parameter, not the colours, the radius, the camera or the sun; the
# cumulative one's after the heights, the exaggeration, the observers' vertices or the radius in cells -- its key is the LIST of
# vertices, compared bit for bit (DESIGN.md 4m item 6 with the cache rule of 4h), so the same observers in another order compute it
# again unless the list of their vertices reads the same (run_case asks the model); the exposure's after the heights, the spacing, the
# exaggeration, a sun, a weight, incidence, softness or bias, not the handle's own sun.  The pyramid is built by the first frame after
# a new image (every set_drape call hands one over) or after enabling, if it has a level above 0, and by nothing else.
STALE_VIEWSHED = ("heights", "exaggeration", "observer_moves", "heights_again", "heights_water")
STALE_CUMULATIVE = ("heights", "exaggeration", "radius", "cumulative_reorder", "heights_again", "heights_water")
STALE_EXPOSURE = ("heights", "exaggeration", "suns_reweight", "incidence_flip", "heights_again", "heights_water")
MIP_BUILDS = ("drape_replace", "drape_opacity_zero")
# the flood and the spill: the two passes between the drape and the exposure tint, flood first.  Their generator is
# default_rng([seed, WATER_STREAM]): no key a case had before them depends on it (digest; tests/test_feature_soak_cases.py pins it)
WATER_STREAM = 0x3A7E2
WATER_PASSES = ("flood", "spill")
WATER_MUTATIONS = ("level", "flood_mode", "spill_mode", "seeds_move", "seeds_nudged", "water_colours_only", "flood_off", "spill_cleared", "heights_water")
FLOOD_MODES = ("everywhere", "edges", "seeds")
SPILL_MODES = ("edges", "seeds")
SEED_COUNTS = (1, 3, 255, 256, 257)                           # k_flood_seed and k_spill_seed run 256 threads a block
LEVEL_QUANTILES = (0.5, 0.3, 0.7, 0.1, 0.9)                   # (in the order of preference among equal shares)
LEVEL_KINDS = ("quantile", "vertex", "below", "above")
DEPTH_FULLS = (0.05, 1.0, 20.0)                               # depth_full over the range of the surface: small, about one, large
WATER_GROUPS = (1, 7, 0)                                      # the group size of the second read of each field; 0: the default, no new scan
# which of the two fields vf_hip.h says a mutation (of any of the three kinds) makes stale, when the field's pass is on.  The flood's
# key is the level's bits, the mode and the list of the seeds' vertices, over the heights; the spill's the mode and the list of its
# seeds' vertices, over the heights.  Neither depends on the colours, depth_full, the camera, the sun or the EXAGGERATION (both fields
# are in units of h before it), nor on a seed that moves inside its vertex's cell; seeds_move makes a field stale where the pass
# takes a seed list and the list of vertices reads differently (run_case asks the model, as for cumulative_reorder).
# vf_terrain_clear_spill frees the field with its buffers (the counter stays), so the next frame after set_spill computes it again
STALE_FLOOD = ("heights", "heights_again", "level", "flood_mode", "seeds_move", "heights_water")
STALE_SPILL = ("heights", "heights_again", "spill_mode", "seeds_move", "spill_cleared", "heights_water")
WATER_KEYS = ("water", "water_mutation", "water_mutation_args")
# hazed overlay layers: which point, line and contour layers take the haze, when their flag is set, a ladder of hazed
# points across the frame's depths, and a mutation of the flags.  Their generator is default_rng([seed, HAZED_STREAM]): no key a
# case had before them depends on it (digest; tests/test_feature_soak_cases.py pins it)
HAZED_STREAM = 0x4A2ED
HAZED_MUTATIONS = ("flag_flip", "flags_all_off", "haze_params", "occlusion_on_hazed", "readd", "polygon_refused")
HAZED_KEYS = ("hazed", "hazed_mutation", "hazed_mutation_args")
FLAG_SHARE = 0.6                                              # the probability of a layer's flag (at least one is set)
LADDER_RUNGS = 12
POLYGON_REFUSED = "a polygon layer cannot take the haze: polygon fills have no depth"
UNKNOWN_LAYER = "no overlay layer with that id"
OLD_KEYS = ("name", "W", "H", "grid", "tex", "amp", "smooth", "nan_texel", "heights", "eye", "target", "fovy", "znear", "zfar", "exaggeration", "spacing", "sun",
            "cmap", "mode", "mutation", "features", "shadows", "ambient", "overlays", "mutation_args", "drape")


def _feed(h, v):
    if isinstance(v, np.ndarray):
        h.update(f"A{v.dtype.str}{v.shape}".encode())
        h.update(np.ascontiguousarray(v).tobytes())
    elif isinstance(v, dict):
        h.update(f"D{len(v)}".encode())
        for k in sorted(v):
            _feed(h, k)
            _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        h.update(f"L{len(v)}".encode())
        for x in v:
            _feed(h, x)
    else:
        if isinstance(v, np.generic):
            v = v.item()
        assert v is None or isinstance(v, (bool, int, float, str)), type(v)
        h.update(f"S{type(v).__name__}:{v!r};".encode())


def digest(cases, keys=OLD_KEYS):
    """sha256 over `keys` of the cases, in order: names, types, values and the bytes of every array (dicts by sorted key)"""
    h = hashlib.sha256()
    for c in cases:
        for k in keys:
            _feed(h, k)
            _feed(h, c[k])
    return h.hexdigest()


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


def vertex_xz(i, j, n, spacing, off=(0.0, 0.0)):
    """world (x, z) of grid vertex (i, j) of n x n, `off` cells beside it"""
    step = 3.0 / (n - 1)
    return float(f32((-1.5 + (i + off[0]) * step) * spacing)), float(f32((-1.5 + (j + off[1]) * step) * spacing))


def snap(c, observer):
    """the vertex (i, j) the library snaps an observer of the case to"""
    return vsm.observer_vertex(observer, max(f32(c["spacing"]), f32(1e-8)), max(c["grid"], 2))


_NEEDS = {"observer_moves": "viewshed", "observer_same_vertex": "viewshed", "radius": "viewshed", "cumulative_reorder": "cumulative",
          "suns_reweight": "exposure", "incidence_flip": "exposure", "haze_off": "haze", "mips_off": "mips", "mips_bias": "mips", "anisotropy": "mips"}


def _late(rng, c, surf, fix, all_on=False):
    """The late passes of a case, from their own generator -> (late, late_mutation, late_mutation_args).  `late`: mips (on / off as
    `on` says), mip_bias, max_anisotropy, the parameters of viewshed, cumulative, exposure and haze as supersample_model.chain takes
    them (cumulative and exposure with the batch size their field is read again at), `on` (which of LATE_PASSES are drawn), supersample.
    fix["late"] is laid over the draw (a dict over a dict key by key); every corner has all passes on (`all_on`).  A seed's mutation
    is the drawn one if it can show in the frame (can_show below), else the next of a drawn order that can."""
    G, sp, W, H = c["grid"], c["spacing"], c["W"], c["H"]
    n = max(G, 2)
    D = c["drape"]
    # a mutation of the mip sampling shows only where an image is left to sample after the case's first mutation
    mips_ok = D is not None and c["mutation"] not in DRAPE_MUTATIONS and D["opacity"] > 0 and min(D["image"].shape[:2]) >= 7 and D["extent_kind"] != "off_grid"
    eligible = [m for m in LATE_MUTATIONS if m not in MIP_MUTATIONS or mips_ok]
    # (the mip mutations are open to fewer cases and get three lots each)
    lots = np.array([3.0 if m in MIP_MUTATIONS else 1.0 for m in eligible])
    kind = eligible[int(rng.choice(len(eligible), p=lots / lots.sum()))]
    kind = fix.get("late_mutation", kind)
    radii = (None, 0.4 * sp, 1.2 * sp, 10.0)
    nanv = np.argwhere(np.isnan(surf))                        # (j, i) of the vertices without a height

    def observers(k):
        return rng.uniform(-1.9 * sp, 1.9 * sp, (k, 2)).astype(f32)       # the terrain spans +-1.5 spacing: beyond it an observer is clamped

    def on_nan():
        j, i = nanv[int(rng.integers(0, len(nanv)))]
        return vertex_xz(int(i), int(j), n, sp)

    def scan():
        return dict(eye_height=float(rng.choice([0.0, 0.05, 1.0])), target_height=float(rng.choice([0.0, 0.02])), softness=float(rng.choice(SOFTNESS)),
                    bias=float(rng.choice([0.0, 0.002, 0.05])))

    def radius(but=()):
        """one of `radii`; `but`: another than these, and a short one unless one of these is short (a change that shows)"""
        short = any(r in radii[1:3] for r in but) or not but
        pick = [r for r in radii if r not in but and (short or r in radii[1:3])]
        return pick[int(rng.integers(0, len(pick)))]

    def colours():
        """(high / visible, low / hidden): the low one mostly with alpha 0, as the defaults have it, so that the tint leaves what
        nobody sees and no sun reaches as it was"""
        return _rgba(rng, int(rng.choice([255, 160, 96, 0], p=[0.3, 0.3, 0.3, 0.1]))), _rgba(rng, int(rng.choice([0, 255, 96], p=[0.6, 0.2, 0.2])))

    def weights(k, up):
        w = rng.random(k).astype(f32)
        if k > 1 and up.any():
            w[int(rng.choice(np.flatnonzero(up)))] = 0.0       # one exact 0, on a sun that counts
        return w

    L = dict(mip_bias=float(rng.choice(MIP_BIASES)), max_anisotropy=int(rng.choice(ANISOTROPIES)))
    o = observers(1)[0]
    if len(nanv) and (rng.random() < 0.5 or fix.get("observer_on_nan")):
        o = on_nan()
    a, b = colours()
    L["viewshed"] = dict(observer=(float(o[0]), float(o[1])), radius=radius(), visible_rgba=a, hidden_rgba=b, **scan())
    N = int(rng.choice(OBSERVER_COUNTS))
    if kind == "cumulative_reorder":
        N = max(N, 7)                                         # (two observers that duplicate each other have one order)
    obs = observers(N)
    order = rng.permutation(N)
    if N > 1:
        obs[order[0]] = obs[order[1]]                         # one duplicates another
    if len(nanv):
        obs[order[-1]] = on_nan()
    a, b = colours()
    # (mostly a short radius: the count is 0 over part of the ground, and the tint leaves it as it was)
    L["cumulative"] = dict(observers=obs, radius=(radii + radii[1:3])[int(rng.integers(0, 6))], high_rgba=a, low_rgba=b, batch=int(rng.choice(OBSERVER_BATCHES)), **scan())
    N = int(rng.choice(SUN_COUNTS))
    # (a day's arc: low suns on one side of the sky, whose shadows overlap and leave part of the ground without any sun)
    el, az = rng.uniform(2.0, 25.0, N), rng.uniform(0.0, 360.0) + rng.uniform(-15.0, 15.0, N)
    if N > 1:
        el[int(rng.integers(0, N))] = -rng.uniform(1.0, 30.0)  # one below the horizon
    a, b = colours()
    L["exposure"] = dict(suns=np.array([shm.sun_vector(e, z) for e, z in zip(el, az)], f32), weights=weights(N, el > 0) if rng.random() < 0.6 else None,
                         incidence=bool(rng.random() < 0.7), softness=float(rng.choice(SOFTNESS)), bias=float(rng.choice([0.0, 0.002, 0.05])),
                         high_rgba=a, low_rgba=b, batch=int(rng.choice(SUN_BATCHES)))
    falloff = [None, 0.3, 4.0][int(rng.integers(0, 3))]
    L["haze"] = dict(density=float(rng.choice([0.05, 0.5, 5.0])), start=float(rng.choice([0.0, 0.5 * float(np.linalg.norm(c["eye"]))])), falloff=falloff,
                     base=float(rng.choice([1.0, 0.6])), max_opacity=float(rng.choice([1.0, 0.6])), background=bool(rng.random() < 0.5), rgba=_rgba(rng))
    on = [p for p in LATE_PASSES if rng.random() < (2.0 / 3.0 if p == "mips" else 0.6)]
    rest = [p for p in rng.permutation(LATE_PASSES) if p not in on]
    on += [str(p) for p in rest[:max(0, 2 - len(on))]]         # at least two
    f = int(rng.choice(FACTORS))
    for k, v in fix.get("late", {}).items():
        L[k] = dict(L[k], **v) if isinstance(v, dict) else v
    f = L.get("supersample", 1 if all_on else f)
    L["supersample"] = 1 if f * max(W, H) > 16384 or f * f * W * H > SAMPLE_CAP else f
    # the mutation's payload (after the corner's own values: an observer moves from where it is)
    V = L["viewshed"]
    v0 = snap(c, V["observer"])
    moved = V["observer"]
    for _ in range(64):
        moved = tuple(float(v) for v in observers(1)[0])
        if snap(c, moved) != v0:
            break
    else:
        moved = vertex_xz(n - 1 - v0[0], n - 1 - v0[1], n, sp)
    same = [p for p in (vertex_xz(v0[0], v0[1], n, sp, off) for off in ((0.2, 0.2), (-0.2, -0.2), (0.2, -0.2), (-0.2, 0.2)))
            if snap(c, p) == v0 and p != tuple(V["observer"])]
    t2 = (int(rng.integers(1, 80)), int(rng.integers(1, 80)))
    E = L["exposure"]
    args = dict({
        "radius": dict(viewshed=radius((V["radius"],)), cumulative=radius((L["cumulative"]["radius"],))),
        "order": np.roll(np.arange(len(L["cumulative"]["observers"])), 1),
        "weights": weights(len(E["suns"]), E["suns"][:, 1] > 0),
        "mip_bias": -16.0 if L["mip_bias"] > 0 else 16.0,
        "max_anisotropy": 16 if L["max_anisotropy"] == 1 else 1,
        "colours": dict(viewshed=colours(), cumulative=colours(), exposure=colours()),
        "heights": _heights(rng, t2, float(rng.choice([0.2, 1.0, 3.0])), bool(rng.random() < 0.5)),
    }, **fix.get("late_mutation_args", {}))
    # A mutation must show in the frame (the two that must not aside; tests/test_feature_soak_cases.py asserts both), so a seed whose
    # drawn one cannot -- by what the vertex field models say of the surface the handle holds after the case's first mutation, no
    # frame needed -- takes the next of a drawn order that can.  A corner's mutation is written down and stays
    h1 = c["mutation_args"]["heights"] if c["mutation"] == "heights" else c["heights"]
    u1 = np.zeros(44, f32)
    u1[36], u1[38] = sp, c["mutation_args"]["exaggeration"] if c["mutation"] == "exaggeration" else c["exaggeration"]

    def tints(hi, lo):
        return tuple(hi) != tuple(lo) and (hi[3] > 0 or lo[3] > 0)

    def can_show(k):
        X = L["exposure"]
        if k == "cumulative_reorder":
            return len(L["cumulative"]["observers"]) >= 7
        if k == "observer_same_vertex":
            return bool(same)
        if k == "anisotropy":                                 # (at a bias of 16 every tap reads the one texel of the coarsest level)
            return L["mip_bias"] < 16.0
        if k in ("heights_again", "radius") and u1[38] == 0.0:   # (a surface without relief is the same under any heights, and all of it
            return False                                      # is seen from anywhere: of a radius only the rim of the disc would move)
        if k in ("observer_moves", "radius"):
            seen = vsm.field(u1, h1, G, V["observer"], **{q: V[q] for q in _SCAN})[0]
            if k == "observer_moves":
                return tints(V["visible_rgba"], V["hidden_rgba"]) and bool((vsm.field(u1, h1, G, moved, **{q: V[q] for q in _SCAN})[0] != seen).any())
            ring = np.logical_xor(*[np.ones((n, n), bool) if r is None else cvm.in_range(n, v0, cvm.rc(r, max(f32(sp), f32(1e-8)), n)) for r in (V["radius"], args["radius"]["viewshed"])])
            return bool((ring & (((seen > 0) & (V["visible_rgba"][3] > 0)) | ((seen < 1) & (V["hidden_rgba"][3] > 0)))).any())
        if k in ("suns_reweight", "incidence_flip"):
            after = dict(X, weights=args["weights"]) if k == "suns_reweight" else dict(X, incidence=not X["incidence"])
            share = []
            for Y in (X, after):
                wtot = sem.weight_total(Y["suns"], Y["weights"])
                if not wtot > 0:
                    return False
                share.append(sem.fraction(sem.field(u1, h1, G, Y["suns"], Y["weights"], incidence=Y["incidence"], softness=Y["softness"], bias=Y["bias"]), wtot))
            return tints(X["high_rgba"], X["low_rgba"]) and bool((share[0] != share[1]).any())
        return True

    if "late_mutation" not in fix:
        order = [eligible[i] for i in rng.permutation(len(eligible))]
        kind = next(k for k in [kind] + order if can_show(k))
    args["observer"] = {"observer_moves": moved, "observer_same_vertex": same[0] if same else tuple(V["observer"])}.get(kind)
    if kind in _NEEDS and _NEEDS[kind] not in on:
        on.append(_NEEDS[kind])
    if kind == "tint_colours_only" and not {"viewshed", "cumulative", "exposure"} & set(on):
        on.append("viewshed")
    L["on"] = LATE_PASSES if all_on else tuple(p for p in LATE_PASSES if p in on)
    return L, kind, args


def seed_vertices(c, seeds):
    """the vertices (N, 2) uint32 the library snaps a seed list of the case to"""
    return fdm.seed_vertices(seeds, max(f32(c["spacing"]), f32(1e-8)), max(c["grid"], 2))


def _sources(c, seeds):
    """a seeds entry (None, "edges" or world (x, z) pairs) as the models' field_heights take it: the list as vertices"""
    return seeds if seeds is None or isinstance(seeds, str) else seed_vertices(c, seeds)


def flood_of(c, surface, F):
    """the flood model's Field of a flood entry on a surface (n, n) of the case's grid"""
    return fdm.field_heights(surface, F["level"], _sources(c, F["seeds"]))


def spill_of(c, surface, S):
    return spm.field_heights(surface, _sources(c, S["seeds"]))


def flood_mode(F):
    return FLOOD_MODES[fdm.mode_of(F["seeds"])]


def spill_mode(S):
    return SPILL_MODES[spm.mode_of(S["seeds"]) - 1]


def surface_at_the_water_mutation(c):
    """the heights the handle holds when run_case applies the water mutation (after the first and the late one), and their surface"""
    h = c["late_mutation_args"]["heights"] if c["late_mutation"] == "heights_again" else c["mutation_args"]["heights"] if c["mutation"] == "heights" else c["heights"]
    return h, cm.surface(h, c["grid"])


def projection(c):
    """(sx, sy, A, B, C, D): the projection of the case's uniform block (u[16:32], column-major) -- clip x = sx x, y = sy y,
    z = A z + B, w = C z + D of a view-space point -- restated from the camera's numbers so that the generator needs no oracle;
    tests/test_feature_soak_cases.py holds it to oracle.look_at_uniforms"""
    sy = 1.0 / math.tan(0.5 * math.radians(c["fovy"]))
    n, f = c["znear"], c["zfar"]
    A = f / (n - f) + 0.5
    return sy * c["H"] / c["W"], sy, A, n * f / (n - f), A - 1.0, n * f / (n - f)


def cut_by_a_clip_plane(c, surface, exaggeration):
    """whether a vertex with a height lies outside 0 <= clip z <= clip w of the case's camera"""
    n = surface.shape[0]
    g = (-1.5 + np.arange(n) * (3.0 / (n - 1))) * c["spacing"]
    X, Z = np.meshgrid(g, g)
    P = np.stack([X, np.nan_to_num(surface.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) * exaggeration, Z], axis=-1)
    f = np.asarray(c["target"], np.float64) - np.asarray(c["eye"], np.float64)
    if not np.linalg.norm(f) > 1e-9:
        return True
    zc = (P - np.asarray(c["eye"], np.float64)) @ (f / np.linalg.norm(f))
    _, _, A, B, C, D = projection(c)
    zcl, wcl = B - A * zc, D - C * zc
    return bool((((wcl <= 0) | (zcl < 0) | (zcl > wcl)) & np.isfinite(surface)).any())


def in_view(c, surface, exaggeration):
    """-> ((n, n) bool, (n, n) int64): the vertices of `surface` that lie in the case's view volume, between the pixel centres of the
    outer columns and rows and half a cell beyond, and the pixel each falls in (row-major; the orientation of the axes does not
    matter to a caller that only asks which vertices share a pixel) -- the camera of oracle.look_at_uniforms (up = +y) in plain
    arithmetic, so that the generator needs no oracle.  A degenerate camera sees nothing."""
    n = surface.shape[0]
    g = (-1.5 + np.arange(n) * (3.0 / (n - 1))) * c["spacing"]
    X, Z = np.meshgrid(g, g)
    P = np.stack([X, np.nan_to_num(surface.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0) * exaggeration, Z], axis=-1)
    eye = np.asarray(c["eye"], np.float64)
    f = np.asarray(c["target"], np.float64) - eye
    r = np.cross(f, (0.0, 1.0, 0.0))
    if not (np.linalg.norm(f) > 1e-9 and np.linalg.norm(r) > 1e-9 * np.linalg.norm(f)):
        return np.zeros((n, n), bool), np.zeros((n, n), np.int64)
    f, r = f / np.linalg.norm(f), r / np.linalg.norm(r)
    u = np.cross(r, f)
    d = P - eye
    zc, xc, yc = d @ f, d @ r, d @ u
    sx, sy, A, B, C, D = projection(c)
    half = 0.5 * 3.0 * c["spacing"] / (n - 1)
    xcl, ycl, zcl, wcl = sx * xc, sy * yc, B - A * zc, D - C * zc       # (view z = -zc: the camera looks down -z)
    inside = ((wcl > 0) & (zcl >= 0) & (zcl <= wcl) & (np.abs(xcl) <= wcl * (1.0 - 1.0 / c["W"]) + half * sx)
              & (np.abs(ycl) <= wcl * (1.0 - 1.0 / c["H"]) + half * sy) & np.isfinite(surface))
    with np.errstate(divide="ignore", invalid="ignore"):
        px = np.clip(np.floor((np.where(inside, xcl / wcl, 0.0) * 0.5 + 0.5) * c["W"]), 0, c["W"] - 1).astype(np.int64)
        py = np.clip(np.floor((np.where(inside, ycl / wcl, 0.0) * 0.5 + 0.5) * c["H"]), 0, c["H"] - 1).astype(np.int64)
    return inside, py * c["W"] + px


_WATER_NEEDS = {"level": "flood", "flood_mode": "flood", "flood_off": "flood", "spill_mode": "spill", "spill_cleared": "spill"}


def _water(rng, c, surf, fix, wish, all_on=False):
    """The flood and the spill of a case, from their own generator -> (water, water_mutation, water_mutation_args).  `water`: `flood`
    (level, seeds, shallow_rgba, deep_rgba, depth_full) and `spill` (the same without the level) as supersample_model.chain takes
    them, `on` (a non-empty subset of WATER_PASSES; every corner has both: `all_on`), level_kind, and for the second read of each
    field flood_group, spill_group and spill_flags.  fix["water"] is laid over the draw (a dict over a dict key by key); there a
    level may be ("vertex", i, j) or ("unique", k) -- that vertex's height, the k-th of the surface's distinct finite heights -- and a
    seeds entry "lowest_corner", "highest" or "on_nan": one seed on that vertex.  The mutation is `wish` (seed % len(WATER_MUTATIONS)
    for a seed) if it can do what it must by what the two models say of the surface the handle holds then and by what the case's
    camera has in view (can_show), else the next of a drawn order that can; fix["water_mutation"] is written down and stays.  The
    pass a mutation needs is switched on for the mutation that is taken, not for the wish."""
    G, sp = c["grid"], c["spacing"]
    n = max(G, 2)
    fin = surf[np.isfinite(surf)]
    lo, hi = (float(fin.min()), float(fin.max())) if fin.size else (0.0, 0.0)
    span = (hi - lo) if hi > lo else 1.0
    nanv = np.argwhere(~np.isfinite(surf))                    # (j, i) of the vertices without a height
    fixed = fix.get("water", {})
    kind = fix.get("water_mutation", wish)

    def at(ji):
        j, i = ji[int(rng.integers(0, len(ji)))]
        return vertex_xz(int(i), int(j), n, sp)

    def seeds():
        """(a seed list, the slots for a seed on a dry vertex): a count from SEED_COUNTS, positions within +-1.9 spacing (beyond +-1.5
        they clamp to the border), one duplicate and one seed on a vertex without a height, if there is one"""
        k = int(rng.choice(SEED_COUNTS))
        s = rng.uniform(-1.9 * sp, 1.9 * sp, (k, 2)).astype(f32)
        order = rng.permutation(k)
        coin = bool(rng.random() < 0.5)
        if k < 3:
            return s, []
        s[order[0]] = s[order[1]]
        if len(nanv) and (k > 3 or coin):
            s[order[-1]] = at(nanv)
        return s, [order[-2]] if k > 3 else [order[-1]] if not (len(nanv) and coin) else []

    def colours():
        """(shallow, deep), as _late's colours(): one of the two sometimes with alpha 0, never both"""
        a, b = _rgba(rng, int(rng.choice([255, 160, 96, 0], p=[0.3, 0.3, 0.3, 0.1]))), _rgba(rng, int(rng.choice([255, 224, 96, 0], p=[0.3, 0.3, 0.3, 0.1])))
        return (a, b) if a[3] or b[3] else (a, b[:3] + (224,))

    def depth_full():
        return max(float(f32(float(rng.choice(DEPTH_FULLS)) * span)), 1e-6)

    def quantiles(surface):
        f = surface[np.isfinite(surface)]
        return [float(f32(np.quantile(f.astype(np.float64), q))) for q in LEVEL_QUANTILES] if f.size else [0.0]

    def named_seed(v):
        if not isinstance(v, str) or v == "edges":
            return v
        if v == "lowest_corner":
            corners = [(0, 0), (n - 1, 0), (0, n - 1), (n - 1, n - 1)]
            i, j = min(corners, key=lambda ij: float(np.nan_to_num(surf[ij[1], ij[0]], nan=np.inf)))
        elif v == "highest":
            j, i = np.argwhere(surf == f32(hi))[0]
        else:
            assert v == "on_nan", v
            j, i = nanv[0]
        return np.array([vertex_xz(int(i), int(j), n, sp)], f32)

    # the draw, all of it for every case (what a later key gets does not depend on which branch an earlier one took)
    fmode, smode = str(rng.choice(FLOOD_MODES)), str(rng.choice(SPILL_MODES, p=[0.6, 0.4]))
    fmode, smode = fixed.get("flood_mode", fmode), fixed.get("spill_mode", smode)
    (fseeds, fdry), (sseeds, _) = seeds(), seeds()
    level_kind = str(rng.choice(LEVEL_KINDS, p=[0.76, 0.08, 0.08, 0.08]))
    pick = int(rng.integers(0, max(fin.size, 1)))
    on = [p for p in WATER_PASSES if rng.random() < 0.7] or [WATER_PASSES[int(rng.integers(0, 2))]]
    (fa, fb), (sa, sb) = colours(), colours()
    over = [float(v) for v in rng.choice(DEPTH_FULLS, 2)]     # depth_full over the surface's range
    W = dict(flood=dict(shallow_rgba=fa, deep_rgba=fb, depth_full=max(float(f32(over[0] * span)), 1e-6)),
             spill=dict(shallow_rgba=sa, deep_rgba=sb, depth_full=max(float(f32(over[1] * span)), 1e-6)), depth_full_over_range=tuple(over),
             flood_group=int(rng.choice(WATER_GROUPS)), spill_group=int(rng.choice(WATER_GROUPS)), spill_flags=bool(rng.random() < 0.6))
    if all_on:
        on = list(WATER_PASSES)

    def on_for(k):
        """the passes that are on if the mutation is k: the drawn ones and the one k needs"""
        return on + [_WATER_NEEDS[k]] if k in _WATER_NEEDS and _WATER_NEEDS[k] not in on else on

    # the two seed mutations need a pass that is on and takes a seed list: where a seed WISHES for one of them and the draw gave none,
    # a mode becomes "seeds", before the level is chosen, and stays so if the mutation then gives way to another
    if kind in ("seeds_move", "seeds_nudged") and "water_mutation" not in fix and not (("flood" in on and fmode == "seeds") or ("spill" in on and smode == "seeds")):
        if "flood" in on:
            fmode = "seeds"
        else:
            smode = "seeds"
    W["flood"]["seeds"] = named_seed(fixed.get("flood", {}).get("seeds", {"everywhere": None, "edges": "edges", "seeds": fseeds}[fmode]))
    W["spill"]["seeds"] = named_seed(fixed.get("spill", {}).get("seeds", {"edges": "edges", "seeds": sseeds}[smode]))
    # the level: usually the quantile of the finite surface under which the flooded share of the wet-able vertices, from the case's own
    # sources, is nearest 0.4 (the flood model's field; no GPU) -- the trick _make uses for the sun's elevation
    level = fixed.get("flood", {}).get("level")
    if isinstance(level, tuple):
        level_kind = "vertex"
        level = float(surf[level[2], level[1]]) if level[0] == "vertex" else float(np.unique(fin)[level[1]])
    elif level is not None:
        level_kind = "fixed"
    elif level_kind == "vertex" and fin.size:
        level = float(fin[pick])
    elif level_kind == "below" and fin.size:
        level = float(f32(lo - max(1.0, 0.01 * abs(lo))))
    elif level_kind == "above" and fin.size:
        level = float(f32(hi + max(1.0, 0.01 * abs(hi))))
    else:
        level_kind = "quantile"
        share = []
        for q in quantiles(surf):
            F = flood_of(c, surf, dict(level=q, seeds=W["flood"]["seeds"]))
            share.append(int(F.flooded.sum()) / max(int(F.wet.sum()), 1))
        # (a level under which the sources flood nothing only where every level is one)
        level = quantiles(surf)[int(np.argmin([abs(v - 0.4) if v > 0 else 1.0 for v in share]))]
    W["flood"]["level"] = level
    dry = np.argwhere(~(surf < f32(level)))
    if fmode == "seeds" and "seeds" not in fixed.get("flood", {}) and len(dry):
        for slot in fdry:                                     # one seed on a dry vertex
            W["flood"]["seeds"][slot] = at(dry)
    for p in WATER_PASSES:
        W[p].update({k: v for k, v in fixed.get(p, {}).items() if k not in ("seeds", "level")})
    for k, v in fixed.items():
        if k not in WATER_PASSES + ("flood_mode", "spill_mode"):
            W[k] = v
    W["level_kind"] = level_kind
    # the mutation's payload, for the surface the handle holds when it comes
    h1, s1 = surface_at_the_water_mutation(c)
    F0, S0 = flood_of(c, s1, W["flood"]), spill_of(c, s1, W["spill"])
    t2 = (int(rng.integers(1, 80)), int(rng.integers(1, 80)))
    (fs2, _), (ss2, _) = seeds(), seeds()                     # the seed lists of a changed mode, and of seeds_move
    (fs3, _), (ss3, _) = seeds(), seeds()

    def nudged(s):
        out = np.array(s, f32)
        for k, v in enumerate(seed_vertices(c, s).tolist()):
            for off in ((0.2, 0.2), (-0.2, -0.2), (0.2, -0.2), (-0.2, 0.2)):
                p = vertex_xz(v[0], v[1], n, sp, off)
                if seed_vertices(c, [p]).tolist() == [v] and p != (float(out[k, 0]), float(out[k, 1])):
                    out[k] = p
                    break
        return out

    seen, pixel = in_view(c, s1, c["mutation_args"]["exaggeration"] if c["mutation"] == "exaggeration" else c["exaggeration"])
    _, held = np.unique(pixel[seen], return_inverse=True)     # per vertex in view: the number of its pixel among those that hold one
    # (where a clip plane cuts the terrain -- a vertex in front of the near or beyond the far plane -- triangles are cut too, and what
    #  the vertices say of the pixels is no guide to which pixels are covered (seed 7011: 174 vertices in view over 66 pixels, 7 pixels covered): every pixel must change there, a fifth elsewhere)
    share = 1 if cut_by_a_clip_plane(c, s1, c["mutation_args"]["exaggeration"] if c["mutation"] == "exaggeration" else c["exaggeration"]) else 5

    def picture(Wt, passes, surface=s1):
        """A coarse picture of what `passes` tint, per vertex: the colour between shallow and deep by depth over depth_full,
        quantised, nothing where the alpha is next to 0.  A mutation that should show has another picture on EVERY vertex of two
        of the pixels that hold a vertex in the camera's view when it comes (in_view: plain arithmetic on the case's camera, no
        frame; of the one such pixel, if there is only one), and of one in five of them (of all of them under a camera whose near or far
        plane cuts the terrain): whatever those pixels show of the surface
        has changed, and the terrain would have to hide four fifths of what the view volume holds to hide them all."""
        out = []
        for p in WATER_PASSES:
            if p in passes and Wt.get(p) is not None:
                M = flood_of(c, surface, Wt[p]) if p == "flood" else spill_of(c, surface, Wt[p])
                depth = M.depth if p == "flood" else M.sink
                t = np.clip(depth / f32(Wt[p]["depth_full"]), 0.0, 1.0)[..., None]
                rgba = np.array(Wt[p]["shallow_rgba"], np.float64) * (1.0 - t) + np.array(Wt[p]["deep_rgba"], np.float64) * t
                rgba[~(depth > 0) | (rgba[..., 3] < 16.0)] = 0.0
                out.append(np.round(rgba / 8.0))
            else:
                out.append(np.zeros((n, n, 4)))
        return np.stack(out)

    def shows(Wt, k):
        passes = on_for(k)
        return score(Wt, passes) >= max(min(2, int(held.max()) + 1), (int(held.max()) + 1 + share - 1) // share) if held.size else False

    def score(Wt, passes):
        """the number of pixels all of whose vertices in view get another picture"""
        if not held.size:
            return 0
        changed = (picture(Wt, passes) != picture(W, passes)).any(axis=(0, 3))[seen]
        return int((np.bincount(held, weights=changed) == np.bincount(held)).sum())

    q1 = quantiles(s1)
    levels = [q for q in (q1[int(i)] for i in rng.permutation(len(q1))) if q != level and shows(dict(W, flood=dict(W["flood"], level=q)), "level")]
    fmodes = [m for name, m in (("everywhere", None), ("edges", "edges"), ("seeds", fs2))
              if name != flood_mode(W["flood"]) and shows(dict(W, flood=dict(W["flood"], seeds=m)), "flood_mode")]
    other = ss2 if spill_mode(W["spill"]) == "edges" else "edges"
    transparent, lot = bool(rng.random() < 0.3), float(rng.random())
    cols = {p: tuple(col[:3] + (0,) for col in colours()) if transparent else colours() for p in WATER_PASSES}
    best = max(q1, key=lambda q: score(dict(W, flood=dict(W["flood"], level=q)), on_for("level")) if q != level else -1)     # (for a corner that names `level`)
    args = dict({
        "level": levels[0] if levels else best if best != level else float(f32(level + 0.25 * span)),
        "flood_seeds": fmodes[int(lot * len(fmodes))] if fmodes else fs2,
        "spill_seeds": other,
        "moved": dict(flood=fs3, spill=ss3),
        "nudged": {p: nudged(W[p]["seeds"]) if isinstance(W[p]["seeds"], np.ndarray) else None for p in WATER_PASSES},
        "colours": cols, "transparent": transparent, "depth_full": dict(flood=depth_full(), spill=depth_full()),
        "heights": _heights(rng, t2, float(rng.choice([0.2, 1.0, 3.0])), bool(rng.random() < 0.5)),
    }, **fix.get("water_mutation_args", {}))

    def listed(p):
        return p in on and isinstance(W[p]["seeds"], np.ndarray)

    def can_show(k):
        if k == "level":
            return bool(levels)
        if k == "flood_mode":
            return bool(fmodes)
        if k == "spill_mode":
            return shows(dict(W, spill=dict(W["spill"], seeds=other)), k)
        if k == "seeds_move":                                 # a new list of vertices, and another picture, for the passes that take a list
            lists = [p for p in WATER_PASSES if listed(p)]
            return (any(seed_vertices(c, args["moved"][p]).tolist() != seed_vertices(c, W[p]["seeds"]).tolist() for p in lists)
                    and shows(dict(W, **{p: dict(W[p], seeds=args["moved"][p]) for p in lists}), k))
        if k == "seeds_nudged":                               # other numbers, the same vertices
            return any(listed(p) and args["nudged"][p].tobytes() != W[p]["seeds"].tobytes()
                       and seed_vertices(c, args["nudged"][p]).tolist() == seed_vertices(c, W[p]["seeds"]).tolist() for p in WATER_PASSES)
        if k == "flood_off":
            return shows(dict(W, flood=None), k)
        if k == "spill_cleared":
            return shows(dict(W, spill=None), k)
        if k == "heights_water":                              # (other ground under the same settings)
            s2 = cm.surface(args["heights"], G)
            return bool((flood_of(c, s2, W["flood"]).flooded != F0.flooded).any() or (_bits(spill_of(c, s2, W["spill"]).sink) != _bits(S0.sink)).any())
        new = {p: dict(W[p], shallow_rgba=cols[p][0], deep_rgba=cols[p][1], depth_full=args["depth_full"][p]) for p in WATER_PASSES}
        return shows(dict(W, **new), k)                       # (the colours: of water that is there)

    if "water_mutation" not in fix:
        order = [WATER_MUTATIONS[i] for i in rng.permutation(len(WATER_MUTATIONS))]
        kind = next((k for k in [kind] + order if can_show(k)), "heights_water")
    W["on"] = tuple(p for p in WATER_PASSES if p in on_for(kind))
    return W, kind, args


def eligible(c):
    """the indices of the case's overlay calls whose layer can take the haze: every call that is not a polygon call"""
    return [k for k, (kind, _) in enumerate(c["overlays"]) if kind != "polygons"]


def ladder_index(c):
    """the layer id of the ladder: it is added after the case's own calls"""
    return len(c["overlays"])


def _ladder(c, rgba, occlude):
    """The ladder of a case (the keywords of a point layer): LADDER_RUNGS draped circles of 5 px on the ground line from under the eye
    through the target to where that line leaves the terrain's square (+-1.5 spacing) -- to twice the target's distance where it
    does not cross the square beyond the target.  Hazed primitives across the frame's depths, whatever the older draw put where."""
    eye, target = np.asarray(c["eye"], np.float64), np.asarray(c["target"], np.float64)
    g0, d = eye[[0, 2]], (target - eye)[[0, 2]]
    if not np.linalg.norm(d) > 1e-9:
        d = np.array([1.0, 0.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        leave = np.where(d != 0.0, (np.sign(d) * 1.5 * c["spacing"] - g0) / d, np.inf).min()
    far = float(leave) if np.isfinite(leave) and leave > 1.0 else 2.0
    t = np.linspace(0.0, far, LADDER_RUNGS)
    xyz = np.column_stack([g0[0] + t * d[0], np.full(LADDER_RUNGS, 0.02), g0[1] + t * d[1]]).astype(f32)
    return dict(xyz=xyz, size_px=5.0, rgba=tuple(rgba), shape="circle", drape=True, occlude=bool(occlude), depth_bias=1e-2)


def haze_at_the_hazed_mutation(c):
    """the haze of the handle when run_case applies the hazed mutation (step H, before the first mutation), or None while it is off"""
    return dict(c["late"]["haze"]) if "haze" in c["late"]["on"] else None


def _hazed(rng, c, fix, wish, parity):
    """Which of a case's layers take the haze, from a generator of its own -> (hazed, hazed_mutation, hazed_mutation_args).  `hazed`:
    flags and early (one bool each per call of eligible(c), in that order: whether the layer is flagged -- at least one is -- and
    whether its flag is set directly after its add, while later layers are still to come, or after all adds) and the ladder (_ladder:
    flagged, opaque, occluding where `parity` is even).  fix["hazed"] is laid over the draw: flags and early as {call index: bool}
    (negative: from the end; a kind's name: every call of that kind), only=True: every flag it does not name is off.  The mutation is `wish` (seed % len(HAZED_MUTATIONS)
    for a seed) if it can do what it must: flag_flip needs the haze on when it comes and a drawn layer that, flagged, covers a pixel
    with S.ah > 0 and whose flip changes the frame of the drawn flags (the model's counts and frames over an empty visibility: no
    oracle frame here, the terrain hides nothing), haze_params the haze on; else the next of a drawn order that can.  fix["hazed_mutation"] is written down and stays."""
    E = eligible(c)
    n = len(c["overlays"])
    fixed = fix.get("hazed", {})
    kind = fix.get("hazed_mutation", wish)
    # the draw, all of it for every case
    flags = [bool(v) for v in rng.random(len(E)) < FLAG_SHARE]
    spare = int(rng.integers(0, len(E)))
    early = [bool(v) for v in rng.random(len(E)) < 0.5]
    colour = _rgba(rng, 255)
    order = [HAZED_MUTATIONS[i] for i in rng.permutation(len(HAZED_MUTATIONS))]
    flip_order = [E[i] for i in rng.permutation(len(E))]
    occ_order = [E[i] for i in rng.permutation(len(E))]
    bias = float(rng.choice([0.0, 1e-2, 0.2]))
    lots = rng.random(3)
    Z = c["late"]["haze"]

    def another(options, now, lot):
        rest = [v for v in options if v != now]
        return rest[int(lot * len(rest))]

    new = dict(density=another((0.05, 0.5, 5.0), Z["density"], lots[0]), start=0.5 * float(np.linalg.norm(c["eye"])) if Z["start"] == 0.0 else 0.0,
               falloff=another((None, 0.3, 4.0), Z["falloff"], lots[1]), rgba=_rgba(rng))
    if not any(flags):
        flags[spare] = True
    if fixed.get("only"):
        flags = [False] * len(E)
    for key, mine in (("flags", flags), ("early", early)):
        for k, v in fixed.get(key, {}).items():               # (a kind's name: every call of that kind)
            for j in [j for j in E if c["overlays"][j][0] == k] if isinstance(k, str) else [k % n]:
                mine[E.index(j)] = bool(v)
    assert any(flags), c["name"]
    H = dict(flags=tuple(flags), early=tuple(early), ladder=_ladder(c, colour, parity % 2 == 0))
    made = []

    def lit(k):
        """whether layer k, flagged alone, covers a pixel with S.ah > 0 under the haze the handle has at step H, the terrain hiding nothing"""
        Zh = haze_at_the_hazed_mutation(c)
        if Zh is None:
            return False
        try:
            u = uniforms(c)
        except RuntimeError:                                  # (a degenerate camera: run() skips the seed)
            return False
        if not made:
            made.append(layers(dict(c, hazed=H), dict(occlusion={}, hazed=dict(flags={}, ladder=False))))
        L = made[0]
        L.set_haze(L.index[k], True)
        blank = np.zeros((c["H"], c["W"]), np.uint32)
        pairs, _, clear = ohm.composite(np.zeros((c["H"], c["W"], 4), np.uint8), blank, u, c["heights"], c["grid"], L, haze=Zh, want_counts=True)[1]
        L.set_haze(L.index[k], False)
        if not pairs > clear:
            return False
        # ... and a later layer does not draw over all of it: the flip changes the frame of the drawn flags (seed 7014's first choice did not)
        frames = []
        for flip in (False, True):
            for j, on in list(zip(E, flags)) + [(n, True)]:
                L.set_haze(L.index[j], on != (flip and j == k))
            frames.append(ohm.composite(np.full((c["H"], c["W"], 4), 128, np.uint8), blank, u, c["heights"], c["grid"], L, haze=Zh))
        for j in E + [n]:
            L.set_haze(L.index[j], False)
        return bool((frames[0] != frames[1]).any())

    chosen = {}

    def can_stand(k):
        if k == "flag_flip":
            chosen["layer"] = next((j for j in flip_order if lit(j)), None)
            return chosen["layer"] is not None
        if k == "haze_params":
            return haze_at_the_hazed_mutation(c) is not None
        return True

    if "hazed_mutation" not in fix:
        kind = next(k for k in [kind] + order if can_stand(k))
    elif kind == "flag_flip" and "layer" not in fix.get("hazed_mutation_args", {}):
        can_stand(kind)                                       # (a corner's flip that names no layer: one that shows, if there is one)
    on = dict(zip(E, flags))
    hazed_pl = [j for j in occ_order if on[j] and c["overlays"][j][0] in ("points", "lines")]
    args = dict({"layer": chosen.get("layer") if chosen.get("layer") is not None else flip_order[0], "haze": new,
                 "occlusion_layer": hazed_pl[0] if hazed_pl else n, "depth_bias": bias}, **fix.get("hazed_mutation_args", {}))
    return H, kind, args


def _make(rng, name, fix, drape_rng, draped=False, late_rng=None, water_rng=None, water_wish=None, hazed_rng=None, hazed_wish=None, parity=0):
    """A case description; `fix` overrides what the draw would choose (CORNERS).  The drape comes from `drape_rng`, a generator of
    its own: what `rng` gives a seed or a corner does not depend on it; `draped`: never without one (every corner).  The late
    passes come from `late_rng` in the same way, the flood and the spill from `water_rng`, the hazed layers from `hazed_rng`."""
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
    c["late"], c["late_mutation"], c["late_mutation_args"] = _late(late_rng, c, surf, fix, all_on=draped)
    c["water"], c["water_mutation"], c["water_mutation_args"] = _water(water_rng, c, surf, fix, water_wish, all_on=draped)
    c["hazed"], c["hazed_mutation"], c["hazed_mutation_args"] = _hazed(hazed_rng, c, fix, hazed_wish, parity)
    return c


def case(seed):
    """The case of a seed: frame, grid, texture, camera and uniforms drawn as test_random_scenes_fuzz draws them, a sun, colormap,
    shade mode, shadow and ambient parameters, which of them are on, the overlay calls, one mutation and (from a generator of its
    own each) a draped image or none, the late passes with their mutation, the flood and the spill with theirs, the hazed layers
    with theirs."""
    return _make(np.random.default_rng(seed), f"seed{seed}", {"mutation": MUTATIONS[seed % len(MUTATIONS)]}, np.random.default_rng([seed, DRAPE_STREAM]),
                 late_rng=np.random.default_rng([seed, LATE_STREAM]), water_rng=np.random.default_rng([seed, WATER_STREAM]),
                 water_wish=WATER_MUTATIONS[seed % len(WATER_MUTATIONS)], hazed_rng=np.random.default_rng([seed, HAZED_STREAM]),
                 hazed_wish=HAZED_MUTATIONS[seed % len(HAZED_MUTATIONS)], parity=seed)


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
    # the late passes of a corner: the haze begins at the eye's distance from its target, about the middle of the terrain's depths, so
    # that it writes part of the frame; a short radius and the incidence cosine leave part of the ground to the other two tints;
    late = {"haze": dict(start=float(np.linalg.norm(np.subtract(base["eye"], base["target"]))), density=0.5),
            "cumulative": dict(radius=0.4 * base["spacing"], high_rgba=cvm.DEFAULT_HIGH, low_rgba=cvm.DEFAULT_LOW),
            # (one low sun, whose long shadows leave part of the ground without any, and one below the horizon)
            "exposure": dict(suns=np.array([shm.sun_vector(6.0, 40.0 * k), shm.sun_vector(-10.0, 40.0 * k + 180.0)], f32), weights=None, incidence=True,
                             high_rgba=sem.DEFAULT_HIGH, low_rgba=sem.DEFAULT_LOW),
            "viewshed": dict(visible_rgba=vsm.DEFAULT_VISIBLE, hidden_rgba=vsm.DEFAULT_HIDDEN)}   # (translucent: no tint hides the passes under it)
    for key, v in fix.get("late", {}).items():
        late[key] = dict(late.get(key, {}), **v) if isinstance(v, dict) else v
    base["late"] = late
    return _make(np.random.default_rng(90000 + k), name, base, np.random.default_rng([90000 + k, DRAPE_STREAM]), draped=True,
                 late_rng=np.random.default_rng([90000 + k, LATE_STREAM]), water_rng=np.random.default_rng([90000 + k, WATER_STREAM]),
                 water_wish=WATER_MUTATIONS[k % len(WATER_MUTATIONS)], hazed_rng=np.random.default_rng([90000 + k, HAZED_STREAM]),
                 hazed_wish=HAZED_MUTATIONS[k % len(HAZED_MUTATIONS)], parity=k)


def _amb(reach, dirs, strength=0.6):
    return dict(strength=strength, reach=float(reach), directions=np.asarray(dirs, f32).reshape(-1, 2))


_FAN = [(-1, 0), (-0.9, 0.31), (-0.9, -0.31)]
_LONG_FOVY = 2.0 * math.degrees(math.atan(0.5 * 1.5 / 6.0))   # from 6 units above, the long side of a frame sees about 0.6 of the terrain's 3 units
# Found by this soak (frame_of_one_column), reduced: a fill whose right edge crosses rows 15-18 at x = 19.4 .. 23.5 of a 17-pixel-wide
# frame -- beyond the frame and inside its last 16-pixel bin column.  k_pg_setup clipped an edge's bins to the frame, the backdrop mask
# gives a bin only the crossings beyond its right edge, so pixel column 16 lost that crossing and the fill
# (tests/test_feature_soak_cases.py asserts where the edge lies).
_BRIDGE = np.full((9, 9), 2.0, f32)                           # (the texture of water_bridge_vertex_at_the_level, below)
_BRIDGE[4, 1:8] = -2.0
_BRIDGE[4, 4] = 0.0
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
    # the late passes' own edges (tests/test_feature_soak_cases.py asserts what each is named for): every pass on,
    # the soak's small frames except where the edge is the frame
    # (the four vertices of grid 2 all see each other: the radius, which reaches along the sides and not across the diagonal, is
    # what shows that the observer moved)
    _corner(30, "late_grid2_observer_on_a_corner_vertex", grid=2, W=33, H=31, tex=(2, 2), ambient=_amb(1.0, _round(4)), late_mutation="observer_moves",
            late=dict(viewshed=dict(observer=(-1.5, -1.5), eye_height=0.05, radius=3.5))),
    _corner(31, "late_grid3_thirty_three_observers", grid=3, W=33, H=31, ambient=_amb(16.0, _FAN), late_mutation="cumulative_reorder",
            late=dict(cumulative=dict(observers=np.random.default_rng(31).uniform(-1.9, 1.9, (33, 2)).astype(f32), batch=3))),
    _corner(32, "late_all_nan_texture", W=33, H=31, heights=np.full((5, 6), np.nan, f32), ambient=_amb(16.0, _round(8)), mutation="heights", late_mutation="suns_reweight",
            late=dict(cumulative=dict(radius=None), exposure=dict(incidence=False))),    # (no radius: every observer counts everywhere; no cosine: that of a NaN is 0)
    _corner(33, "late_observer_on_the_nan_vertex", W=48, H=40, tex=(9, 7), nan_texel=True, ambient=_amb(16.0, _FAN), observer_on_nan=True, late_mutation="observer_same_vertex"),
    _corner(34, "late_exaggeration0_eye_height0", W=48, H=40, exaggeration=0.0, ambient=_amb(16.0, _round(8)), mutation="exaggeration", mutation_args={"exaggeration": 1.5},
            late_mutation="tint_colours_only", late=dict(viewshed=dict(eye_height=0.0), cumulative=dict(eye_height=0.0))),
    _corner(35, "late_exaggeration_minus2", W=48, H=40, exaggeration=-2.0, ambient=_amb(16.0, _FAN), late_mutation="heights_again"),
    _corner(36, "late_frame_of_one_column", W=1, H=70, grid=17, ambient=_amb(16.0, _FAN), late_mutation="incidence_flip"),
    # (a field of view of 0.3 degrees over the one row's height: its 130 pixels run across the terrain through the target)
    _corner(37, "late_frame_of_one_row", W=130, H=1, grid=16, fovy=0.3, ambient=_amb(1.5, _round(3)), late_mutation="haze_off"),
    # the camera of drape_near_plane_through_the_terrain: the tints and the haze read the interpolated position of clipped primitives
    _corner(38, "late_near_plane_through_the_terrain", grid=9, eye=(0.9, 0.7, 0.8), target=(-0.4, -0.2, -0.3), znear=0.4, fovy=60.0,
            ambient=_amb(16.0, _FAN, strength=0.6), late_mutation="radius",
            drape=dict(image=distinct_image(37, 64), extent=(-0.9, -1.0, 0.6, 0.7), extent_kind="interior", opacity=0.37, filter="linear"),
            late=dict(viewshed=dict(observer=(-0.4, -0.3), eye_height=1.0, radius=None, visible_rgba=(40, 250, 90, 160), hidden_rgba=(250, 30, 30, 96)),
                      cumulative=dict(radius=None, high_rgba=(30, 60, 250, 160), low_rgba=(0, 0, 0, 0)), haze=dict(start=0.0, density=0.5, falloff=None))),
    _corner(39, "late_sky_camera_haze_on_the_background", W=48, H=40, eye=(3.0, 2.0, 3.0), target=(3.6, 4.0, 3.4), ambient=_amb(16.0, _FAN), late_mutation="haze_off",
            late=dict(haze=dict(background=True, rgba=(200, 215, 235, 255), max_opacity=0.6))),
    _corner(40, "late_every_sun_below_the_horizon", W=48, H=40, ambient=_amb(16.0, _FAN), late_mutation="tint_colours_only",
            late=dict(exposure=dict(suns=np.array([shm.sun_vector(-5.0, 20.0), shm.sun_vector(-40.0, 200.0), (0.3, 0.0, 1.0)], f32), weights=None))),
    # (a cell of grid 9 is 0.375 wide: a disc of some six pixels around the observer's vertex)
    _corner(41, "late_radius_below_one_cell", grid=9, ambient=_amb(16.0, _FAN), late_mutation="observer_moves",
            late=dict(viewshed=dict(radius=0.3, observer=(0.1, -0.2), visible_rgba=(40, 250, 90, 255)), cumulative=dict(radius=0.3))),
    _corner(42, "late_drape_1x1_mips_on", W=48, H=40, ambient=_amb(16.0, _FAN), mutation="sun", late_mutation="observer_moves",
            drape=dict(image=np.array([[(200, 90, 33, 180)]], np.uint8), extent=None, extent_kind="whole", opacity=1.0, filter="linear")),
    _corner(43, "late_dense_drape_bias_minus16", W=15, H=17, ambient=_amb(16.0, _FAN), mutation="sun", late_mutation="mips_bias", late_mutation_args={"mip_bias": 3.0},
            late=dict(mip_bias=-16.0, max_anisotropy=1),
            drape=dict(image=dmm.case_image(43, (300, 300)), extent=None, extent_kind="whole", opacity=1.0, filter="linear")),
    _corner(44, "late_dense_drape_bias_16", W=15, H=17, ambient=_amb(16.0, _FAN), mutation="sun", late_mutation="mips_bias", late_mutation_args={"mip_bias": -16.0},
            late=dict(mip_bias=16.0, max_anisotropy=1),
            drape=dict(image=dmm.case_image(43, (300, 300)), extent=None, extent_kind="whole", opacity=1.0, filter="linear")),
    _corner(45, "late_anisotropy16_grazing_camera", W=48, H=40, eye=(3.2, 0.45, 0.3), ambient=_amb(16.0, _FAN), mutation="sun", late_mutation="anisotropy",
            late=dict(mip_bias=0.0, max_anisotropy=16),
            # (the image stretched sixteenfold along z under the low eye: footprints longer than sixteen times their width)
            drape=dict(image=dmm.case_image(45, (300, 256)), extent=(-1.5, -24.0, 1.5, 24.0), extent_kind="stretched", opacity=1.0, filter="linear")),
    _corner(46, "late_supersample4_frame1x1", W=1, H=1, ambient=_amb(16.0, _FAN), late_mutation="incidence_flip", late=dict(supersample=4)),
    _corner(47, "late_supersample3_frame15x17", W=15, H=17, ambient=_amb(16.0, _FAN), mutation="sun", late_mutation="mips_off",
            late=dict(supersample=3, max_anisotropy=8, mip_bias=0.0),
            drape=dict(image=dmm.case_image(43, (300, 300)), extent=None, extent_kind="whole", opacity=1.0, filter="linear")),
    # the flood's and the spill's own edges (tests/test_feature_soak_cases.py asserts what each is named for): both
    # passes on, small frames.  Below grid 64 most lanes and registers of the one 64 x 64 tile lie beyond the grid
    _corner(50, "water_grid2_all_border", grid=2, W=33, H=31, tex=(2, 2), ambient=_amb(1.0, _round(4)), water_mutation="level",
            water=dict(flood=dict(seeds="edges", level=("unique", -1)), spill=dict(seeds="edges"))),
    # (from the lowest corner vertex; the centre's height is the level, and `h < level` is strict: it stays dry)
    _corner(51, "water_grid3_centre_at_the_level", grid=3, W=33, H=31, ambient=_amb(16.0, _FAN), water_mutation="level",
            water=dict(flood=dict(seeds="lowest_corner", level=("vertex", 1, 1)), spill=dict(seeds="lowest_corner"))),
    # white noise of amplitude 3, a texel a vertex and more: sinks by the thousand; a tile short by one row and column, and a whole one
    _corner(52, "water_grid63_white_noise", grid=63, tex=(79, 79), smooth=False, amp=3.0, ambient=_amb(16.0, _FAN), water_mutation="spill_mode",
            water=dict(flood=dict(seeds="edges"), spill=dict(seeds="edges"))),
    _corner(53, "water_grid64_white_noise", grid=64, tex=(79, 79), smooth=False, amp=3.0, ambient=_amb(16.0, _FAN), water_mutation="spill_cleared",
            water=dict(flood=dict(seeds="edges"), spill=dict(seeds="edges"))),
    # 3 x 3 tiles, the outer ones two vertices wide, one seed in the middle of the first: the water crosses tile borders pass by pass
    # while the tiles it has left rest
    _corner(54, "water_grid130_white_noise_from_one_seed", grid=130, tex=(130, 130), smooth=False, amp=3.0, ambient=_amb(16.0, _FAN), water_mutation="seeds_move",
            # (the level well above the site-percolation threshold of the noise: the water from the seed crosses the grid)
            water=dict(flood=dict(seeds=np.array([vertex_xz(20, 20, 130, 1.0)], f32), level=0.6), spill=dict(seeds=np.array([vertex_xz(20, 20, 130, 1.0)], f32)),
                       flood_group=1, spill_group=7, spill_flags=False),
            water_mutation_args={"moved": dict(flood=np.array([vertex_xz(120, 70, 130, 1.0)], f32), spill=np.array([vertex_xz(120, 70, 130, 1.0)], f32))}),
    # nothing is wet-able or passable: counts of 0, a spill of +inf, a sink depth of 0, the frame as it was; the heights mutation brings
    # ground, and both fields are computed again
    _corner(55, "water_all_nan_texture", W=33, H=31, heights=np.full((5, 6), np.nan, f32), ambient=_amb(16.0, _round(8)), mutation="heights",
            late_mutation="tint_colours_only", water_mutation="flood_off", water=dict(flood=dict(seeds="edges", level=0.0), spill=dict(seeds="edges"))),
    # the only seed of either pass on the one vertex without a height: no source, nothing flooded or reached; heights_water brings one
    _corner(57, "water_only_seed_on_the_nan_vertex", W=48, H=40, tex=(9, 7), nan_texel=True, ambient=_amb(16.0, _FAN), late_mutation="tint_colours_only",
            water_mutation="heights_water", water=dict(flood=dict(seeds="on_nan", level=5.0), spill=dict(seeds="on_nan"))),   # (the level above the new heights too: the seed's vertex is wet then)
    # the staircase of constant_texture_level_on_the_plateau: nine distinct heights, consecutive binary32 numbers.  The level is the
    # middle one (a tie with every vertex of that plateau, all dry); the spill comes from a seed on the highest plateau, so the ties
    # below it hold sinks -- from the border there are none
    _corner(58, "water_plateau_of_ties", heights=np.full((4, 4), 2.0 ** 20, f32), exaggeration=2.0 ** -20, ambient=_amb(16.0, _round(8)), mutation="sun",
            late_mutation="tint_colours_only", water_mutation="spill_mode",
            water=dict(flood=dict(seeds="edges", level=("unique", 4), depth_full=0.25), spill=dict(seeds="highest", depth_full=0.25))),
] + [
    # the level above everything (all the finite ground is wet-able) and below everything (none is), in each of the three modes
    _corner(60 + 3 * a + m, f"water_level_{where}_everything_{FLOOD_MODES[m]}", W=48, H=40, ambient=_amb(16.0, _FAN), water_mutation="level",
            water=dict(flood_mode=FLOOD_MODES[m], flood=dict(level=lv)))
    for a, (where, lv) in enumerate((("above", 1e6), ("below", -1e6))) for m in range(3)
] + [
    # neither field depends on the exaggeration: none is computed again, and the tints follow the surface the frame draws
    _corner(70, "water_exaggeration0_then_minus2", W=48, H=40, exaggeration=0.0, ambient=_amb(16.0, _round(8)), mutation="exaggeration",
            mutation_args={"exaggeration": -2.0}, late_mutation="tint_colours_only", water_mutation="water_colours_only"),
    # the camera of late_near_plane_through_the_terrain: the CLIPPED instantiation of both tint kernels
    _corner(71, "water_near_plane_through_the_terrain", grid=9, eye=(0.9, 0.7, 0.8), target=(-0.4, -0.2, -0.3), znear=0.4, fovy=60.0,
            ambient=_amb(16.0, _FAN, strength=0.6), late_mutation="tint_colours_only", water_mutation="flood_off",
            water=dict(flood=dict(seeds=None, level=0.4, shallow_rgba=(96, 176, 224, 160), deep_rgba=(16, 64, 160, 224)),
                       spill=dict(seeds=np.array([(1.4, 1.4)], f32), shallow_rgba=(255, 224, 64, 160), deep_rgba=(160, 32, 16, 240)))),
    # (the level above everything: the one pixel is under water, whichever vertex it shows)
    _corner(72, "water_frame1x1", W=1, H=1, ambient=_amb(16.0, _FAN), water_mutation="flood_off", water=dict(flood=dict(seeds=None, level=1e6, deep_rgba=(16, 64, 160, 224)))),
    _corner(73, "water_frame_of_one_column", W=1, H=70, grid=17, ambient=_amb(16.0, _FAN), water_mutation="spill_cleared", water=dict(flood=dict(seeds=None))),
    _corner(74, "water_frame_of_one_row", W=130, H=1, grid=16, fovy=0.3, ambient=_amb(1.5, _round(3)), water_mutation="flood_off", water=dict(flood=dict(seeds=None))),
    _corner(75, "water_supersample3_frame15x17", W=15, H=17, ambient=_amb(16.0, _FAN), mutation="sun", late_mutation="tint_colours_only",
            water_mutation="level", late=dict(supersample=3), water=dict(flood=dict(seeds="edges"))),
    # a texel a vertex: walls, and a channel along row 4 whose middle vertex lies exactly at the level.  `h < level` is strict, so the
    # water from the seed at the channel's one end stops in front of it and the other half stays dry: a kernel that takes `<=` floods
    # the whole channel, and the field and the frame show it, not the counts alone
    # (corner 87: its drawn overlays leave the channel in sight; tests/test_feature_soak_cases.py asserts that the whole frame shows it)
    _corner(87, "water_bridge_vertex_at_the_level", grid=9, heights=_BRIDGE, exaggeration=0.05, ambient=_amb(16.0, _FAN), mutation="sun",
            late_mutation="tint_colours_only", water_mutation="flood_mode", water_mutation_args={"flood_seeds": None},
            water=dict(flood=dict(seeds=np.array([vertex_xz(1, 4, 9, 1.0)], f32), level=("vertex", 4, 4), shallow_rgba=(96, 176, 224, 200), deep_rgba=(16, 64, 160, 240)),
                       spill=dict(seeds=np.array([vertex_xz(1, 4, 9, 1.0)], f32)))),
]
OLD_CORNERS = 29                                             # the corners older than the late passes: their old keys are pinned (digest)
LATE_CORNERS = 47                                             # ... and those older than the flood and the spill: theirs and their late keys
WATER_CORNERS = 68                                            # ... and those older than the hazed layers: all their keys but the hazed ones


# the hazed layers' own edges (tests/test_feature_soak_cases.py asserts what each is named for): every pass on, small
# frames.  A corner's own layers follow the eight drawn calls (DRAWN + j) or, where the record counts matter, replace them
DRAWN = 8


def _hz(**kw):
    """the haze of a hazed corner: from the eye on, uniform, opaque at most, unless `kw` says otherwise"""
    return dict(haze=dict(dict(start=0.0, density=0.3, falloff=None, base=0.0, max_opacity=1.0, rgba=(200, 215, 235, 255), background=False), **kw))


def _pts(xyz, size_px, drape, rgba=(255, 60, 40, 255), shape="circle", occlude=False, depth_bias=1e-2):
    return ("points", dict(xyz=np.asarray(xyz, f32).reshape(-1, 3), size_px=size_px, rgba=rgba, shape=shape, drape=drape, occlude=occlude, depth_bias=depth_bias))


def _lns(paths, width_px, cap, drape, rgba=(250, 220, 30, 255), occlude=False, depth_bias=1e-2):
    return ("lines", dict(paths=[np.asarray(p, f32).reshape(-1, 3) for p in paths], width_px=width_px, rgba=rgba, cap=cap, drape=drape, occlude=occlude,
                          depth_bias=depth_bias))


def _own(*flags, early=()):
    """the `hazed` entry of a corner: only its own layers DRAWN + j, j in `flags`, take the haze; those in `early` directly after their add"""
    return dict(only=True, flags={DRAWN + j: True for j in flags}, early={DRAWN + j: j in early for j in flags})


_P, _Q = (0.3, 0.3, 0.2), (-0.8, 0.1, 0.6)
_EYE, _TARGET = np.array(_CAMERA["eye"]), np.array(_CAMERA["target"])
_BEHIND = _EYE + 0.7 * (_EYE - _TARGET) + [0.01, 0.02, 0.03]  # (as _overlays draws it: from the target to behind the eye)
_THROUGH_THE_EYE = [_lns([[_TARGET, _BEHIND]], 7.0, "round", False), _lns([[(0.0, 0.02, 0.0), (_BEHIND[0], 0.02, _BEHIND[2])]], 3.0, "butt", True, rgba=(40, 250, 90, 255))]
_NEAR = dict(grid=9, eye=(0.9, 0.7, 0.8), target=(-0.4, -0.2, -0.3), znear=0.4, fovy=60.0)     # (the camera of drape_near_plane_through_the_terrain)
_LATTICE = np.array([(x, 0.02, z) for x in np.linspace(-1.4, 1.4, 9) for z in np.linspace(-1.4, 1.4, 9)], f32)
_ACROSS = [(-1.4, 0.02, -1.2), (0.0, 0.02, 0.1), (1.4, 0.02, 1.3)]
_NOISE = dict(grid=65, tex=(65, 65), smooth=False, amp=1.0, W=96, H=64)
_CLOUD = np.random.default_rng(110).uniform(-1.4, 1.4, (300, 3)).astype(f32) * np.array([1.0, 0.0, 1.0], f32) + np.array([0.0, 0.02, 0.0], f32)
_SIX_LEVELS = ("contours", dict(levels=np.linspace(-0.3, 0.3, 6).astype(f32), width_px=1.0, rgba=(20, 20, 20, 255), lift=0.0, join="round", occlude=False, depth_bias=1e-2))
_PATCH = ("polygons", dict(polygons=[[_ring((0.2, -0.1), 0.5, 5, 0.02)]], fill_rgba=(0, 90, 255, 150), line_rgba=(0, 0, 0, 255), line_width_px=1.0, drape=True))
_BIG = [_pts([(0.0, 0.02, 0.0)], 64.0, True), _lns([[(-1.0, 0.02, -1.0), (1.0, 0.02, 1.0)]], 80.0, "round", True)]
_SPECS += [
    # a zero-length segment under every cap, alone in its path and in front of a longer one, half a pixel and 80 pixels wide
    _corner(100, "hazed_zero_length_segments_every_cap", ambient=_amb(16.0, _FAN), late=_hz(falloff=4.0), hazed_mutation="flag_flip", hazed_mutation_args={"layer": DRAWN + 2},
            more_overlays=[_lns([[_P, _P], [_P, _P, _Q]], w, cap, False, rgba=(250, 40 + 90 * j, 30, 255)) for w in (80.0, 0.5) for j, cap in enumerate(CAPS)],
            hazed=_own(0, 1, 2, 3, 4, 5, early=(0, 3))),
    # a free and a draped path from the target to behind the eye under a shallow layer of haze: the clipped end's interpolated y decides
    # the opacity; then under fovy 170 and a density of 5, where it saturates at max_opacity
    _corner(101, "hazed_paths_through_the_eye_falloff0p3", ambient=_amb(16.0, _FAN), late=_hz(falloff=0.3, density=0.5), hazed_mutation="haze_params",
            more_overlays=_THROUGH_THE_EYE, hazed=_own(0, 1, early=(0,))),
    _corner(102, "hazed_paths_through_the_eye_fovy170_saturated", fovy=170.0, ambient=_amb(16.0, _FAN), late=_hz(falloff=0.3, density=5.0, max_opacity=0.6),
            hazed_mutation="flags_all_off", more_overlays=_THROUGH_THE_EYE, hazed=_own(0, 1)),
    # the near plane through the terrain: a hazed occluding layer beside an unhazed occluding one (ov_terrain_rw on clipped triangles)
    _corner(103, "hazed_near_plane_through_the_terrain", **_NEAR, ambient=_amb(16.0, _FAN, strength=0.6), late=_hz(density=0.5), hazed_mutation="occlusion_on_hazed",
            hazed_mutation_args={"occlusion_layer": DRAWN, "depth_bias": 0.0},
            more_overlays=[_pts(_LATTICE, 6.0, True, occlude=True), _lns([_ACROSS], 3.0, "round", True, occlude=True, depth_bias=0.0)], hazed=_own(0, early=(0,))),
    # draped hazed points and a draped hazed path over vertices without a height: what is drawn is what the model says
    _corner(104, "hazed_draped_over_one_nan_texel", tex=(9, 7), nan_texel=True, ambient=_amb(16.0, _FAN), late=_hz(falloff=4.0), hazed_mutation="flag_flip",
            hazed_mutation_args={"layer": DRAWN}, more_overlays=[_pts(_LATTICE, 6.0, True), _lns([_ACROSS], 3.0, "square", True)], hazed=_own(0, 1, early=(1,))),
    _corner(105, "hazed_draped_over_the_all_nan_texture", heights=np.full((5, 6), np.nan, f32), ambient=_amb(16.0, _round(8)), mutation="heights", late=_hz(falloff=4.0),
            hazed_mutation="readd", more_overlays=[_pts(_LATTICE, 6.0, True), _lns([_ACROSS], 3.0, "square", True)], hazed=_own(0, 1)),
] + [
    # no opacity, three ways: the frame is the unflagged bytes; haze_params brings `start` to 0
    _corner(106 + j, f"hazed_no_opacity_{name}", ambient=_amb(16.0, _FAN), late=_hz(**kw), hazed_mutation="haze_params",
            hazed_mutation_args={"haze": dict(density=0.5, start=0.0, falloff=None, rgba=(200, 215, 235, 255))},
            more_overlays=[_pts(_LATTICE, 6.0, True), _lns([_ACROSS], 3.0, "round", False)], hazed=_own(0, 1, early=(0,)))
    for j, (name, kw) in enumerate((("start_beyond_every_depth", dict(start=1e6)), ("max_opacity_0", dict(max_opacity=0.0)), ("colour_of_alpha_0", dict(rgba=(200, 215, 235, 0)))))
] + [
    # the side array behind its allocation: one point flagged early, then a contour layer of six levels over white noise -- thousands of
    # GPU-extracted records -- flagged late, then 300 one-pixel points; and every layer unflagged until one flag on the last
    _corner(110, "hazed_side_array_grows_behind_an_early_flag", **_NOISE, ambient=_amb(16.0, _FAN), late=_hz(falloff=4.0), hazed_mutation="flag_flip",
            hazed_mutation_args={"layer": 1}, overlays=[_pts([(0.1, 0.02, -0.2)], 9.0, True), _SIX_LEVELS, _pts(_CLOUD, 1.0, True, rgba=(255, 255, 255, 255)), _PATCH],
            mutation_args={"layer": 0}, hazed=dict(flags={0: True, 1: True, 2: True}, early={0: True, 1: False, 2: False})),
    _corner(111, "hazed_one_flag_on_the_last_layer", **_NOISE, ambient=_amb(16.0, _FAN), late=_hz(falloff=4.0), hazed_mutation="readd",
            overlays=[_pts([(0.1, 0.02, -0.2)], 9.0, True), _SIX_LEVELS, _PATCH, _pts(_CLOUD, 1.0, True, rgba=(255, 255, 255, 255))],
            mutation_args={"layer": 0}, hazed=dict(only=True, flags={3: True}, early={3: False})),
    # the contour layer of the 2^20 staircase, a level on a plateau, hazed; the height upload comes under its snapshot
    _corner(112, "hazed_contours_on_the_staircase", heights=np.full((4, 4), 2.0 ** 20, f32), exaggeration=2.0 ** -20, ambient=_amb(16.0, _round(8)), mutation="heights",
            late=_hz(falloff=4.0), hazed_mutation="flags_all_off", hazed=dict(only=True, flags={"contours": True}, early={"contours": True})),
    # frames of one pixel, one column and one row under a 64-px point and an 80-px line
    _corner(113, "hazed_frame1x1", W=1, H=1, ambient=_amb(16.0, _FAN), late=_hz(), hazed_mutation="flags_all_off", more_overlays=_BIG, hazed=_own(0, 1)),
    _corner(114, "hazed_frame_of_one_column", W=1, H=70, grid=17, ambient=_amb(16.0, _FAN), late=_hz(), hazed_mutation="occlusion_on_hazed",
            hazed_mutation_args={"occlusion_layer": DRAWN + 1}, more_overlays=_BIG, hazed=_own(0, 1, early=(0,))),
    _corner(115, "hazed_frame_of_one_row", W=130, H=1, grid=16, fovy=0.3, ambient=_amb(1.5, _round(3)), late=_hz(), hazed_mutation="polygon_refused",
            more_overlays=_BIG, hazed=_own(0, 1, early=(1,))),
    # supersampled handles take the flags and the ladder
    _corner(116, "hazed_supersample3_frame15x17", W=15, H=17, ambient=_amb(16.0, _FAN), mutation="sun", late=dict(_hz(falloff=4.0), supersample=3), hazed_mutation="flag_flip",
            hazed=dict(flags={"points": True, "lines": True, "contours": True})),
    _corner(117, "hazed_supersample4_frame1x1", W=1, H=1, ambient=_amb(16.0, _FAN), late=dict(_hz(), supersample=4), hazed_mutation="haze_params",
            water_mutation="seeds_nudged", water=dict(spill=dict(seeds=np.array([(0.1, 0.1)], f32))),      # (a water mutation that must not show: one pixel shows little)
            more_overlays=_BIG, hazed=dict(flags={"points": True, "lines": True, "contours": True, DRAWN: True, DRAWN + 1: True})),
    # no relief and a narrow grid, an inverted relief and a wide one: a draped and a free hazed layer each
    _corner(118, "hazed_exaggeration0_spacing0p3", exaggeration=0.0, spacing=0.3, ambient=_amb(16.0, _round(8)), mutation="exaggeration", mutation_args={"exaggeration": -2.0},
            late=_hz(density=1.0), hazed_mutation="occlusion_on_hazed", hazed_mutation_args={"occlusion_layer": DRAWN},
            more_overlays=[_pts(_LATTICE * f32(0.3), 6.0, True), _lns([np.array(_ACROSS) * 0.3 + [0.0, 0.1, 0.0]], 3.0, "round", False)], hazed=_own(0, 1, early=(0,))),
    _corner(119, "hazed_exaggeration_minus2_spacing2p5", exaggeration=-2.0, spacing=2.5, amp=0.2, ambient=_amb(16.0, _FAN), mutation="exaggeration", late=_hz(density=0.1),
            hazed_mutation="readd", more_overlays=[_pts(_LATTICE * f32(2.5), 6.0, True), _lns([np.array(_ACROSS) * 2.5 + [0.0, 0.3, 0.0]], 3.0, "round", False)],
            hazed=_own(0, 1, early=(1,))),
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
                overlays=False, occlusion={}, drape=None, late=None, water=None, hazed=None)


def hazed_on(c, state, flags=None):
    """the state with the case's layers flagged as its `hazed` entry says and the ladder added behind them (run_case's step 4):
    hazed = dict(flags: {call index: bool} of eligible(c), ladder: the ladder's flag); None: no flag, no ladder.  `flags`: every
    flag, the ladder's too, takes this value instead"""
    F = c["hazed"]["flags"] if flags is None else [flags] * len(c["hazed"]["flags"])
    return dict(state, hazed=dict(flags=dict(zip(eligible(c), F)), ladder=True if flags is None else flags))


def hazed_steps(c, state):
    """The states (overlays on, the flags and the ladder in `hazed`) the case's hazed mutation leads through, in order: [(what,
    state)].  One for every mutation but readd: every call added again unflagged, then again with the flags as they were.
    polygon_refused leaves the state as it is."""
    kind, a = c["hazed_mutation"], c["hazed_mutation_args"]
    Hz = dict(state["hazed"], flags=dict(state["hazed"]["flags"]))
    s = dict(state, hazed=Hz)
    if kind == "flag_flip":
        Hz["flags"][a["layer"]] = not Hz["flags"][a["layer"]]
    elif kind == "flags_all_off":
        return [(kind, hazed_on(c, state, flags=False))]
    elif kind == "haze_params":
        s["late"] = dict(state["late"], haze=dict(state["late"]["haze"], **a["haze"]))
    elif kind == "occlusion_on_hazed":
        k = a["occlusion_layer"]
        now = state["occlusion"][k][0] if k in state["occlusion"] else (c["hazed"]["ladder"] if k == ladder_index(c) else c["overlays"][k][1])["occlude"]
        s["occlusion"] = {**state["occlusion"], k: (not now, a["depth_bias"])}
    elif kind == "readd":
        again = dict(state, occlusion={})
        return [("every call added again, unflagged", hazed_on(c, again, flags=False)), ("added again, the flags set the other way round", dict(again, hazed=Hz))]
    return [(kind, s)]


def hazed_mutated(c, state):
    """the state after the case's hazed mutation"""
    return hazed_steps(c, state)[-1][1]


def watered(c, state):
    """the state with the case's flood and spill on (those of `on`): for each its parameters, or None while it is off; `cleared`:
    clear_spill was the last call for the spill"""
    P = c["water"]
    return dict(state, water=dict(cleared=False, **{p: {k: v for k, v in P[p].items()} if p in P["on"] else None for p in WATER_PASSES}))


def water_steps(c, state):
    """The states (with the water on) the case's water mutation leads through, in order: [(what, state)].  One for every mutation
    but spill_cleared: the spill cleared, then set again as it was.  A mutation of a pass that is off changes nothing of it."""
    kind, a = c["water_mutation"], c["water_mutation_args"]
    Wt = dict(state["water"])
    s = dict(state, water=Wt)
    F, S = Wt["flood"], Wt["spill"]

    def listed(P):
        return P is not None and isinstance(P["seeds"], np.ndarray)

    if kind == "level":
        Wt["flood"] = dict(F, level=a["level"])
    elif kind == "flood_mode":
        Wt["flood"] = dict(F, seeds=a["flood_seeds"])
    elif kind == "spill_mode":
        Wt["spill"] = dict(S, seeds=a["spill_seeds"])
    elif kind in ("seeds_move", "seeds_nudged"):
        for p in WATER_PASSES:
            if listed(Wt[p]):
                Wt[p] = dict(Wt[p], seeds=a["moved" if kind == "seeds_move" else "nudged"][p])
    elif kind == "water_colours_only":
        for p in WATER_PASSES:
            if Wt[p] is not None:
                Wt[p] = dict(Wt[p], shallow_rgba=a["colours"][p][0], deep_rgba=a["colours"][p][1], depth_full=a["depth_full"][p])
    elif kind == "flood_off":
        Wt["flood"] = None
    elif kind == "spill_cleared":
        return [("spill cleared", dict(state, water=dict(Wt, spill=None, cleared=True))), ("spill set again", s)]
    elif kind == "heights_water":
        s["heights"] = a["heights"]
    return [(kind, s)]


def water_mutated(c, state):
    """the state after the case's water mutation"""
    return water_steps(c, state)[-1][1]


def lated(c, state):
    """the state with the case's late passes on: mips (with the bias), max_anisotropy, and for each of viewshed, cumulative,
    exposure and haze its parameters, or None while it is off"""
    L = c["late"]
    return dict(state, late=dict(mips="mips" in L["on"], mip_bias=L["mip_bias"], max_anisotropy=L["max_anisotropy"],
                                 **{p: dict(L[p]) if p in L["on"] else None for p in LATE_PASSES[1:]}))


def late_mutated(c, state):
    """the state (with its late passes on) after the case's late mutation"""
    kind, a = c["late_mutation"], c["late_mutation_args"]
    L = dict(state["late"])
    s = dict(state, late=L)
    if kind in ("observer_moves", "observer_same_vertex"):
        L["viewshed"] = dict(L["viewshed"], observer=a["observer"])
    elif kind == "radius":
        L["viewshed"] = dict(L["viewshed"], radius=a["radius"]["viewshed"])
        if L["cumulative"] is not None:
            L["cumulative"] = dict(L["cumulative"], radius=a["radius"]["cumulative"])
    elif kind == "cumulative_reorder":
        L["cumulative"] = dict(L["cumulative"], observers=np.ascontiguousarray(L["cumulative"]["observers"][a["order"]]))
    elif kind == "suns_reweight":
        L["exposure"] = dict(L["exposure"], weights=a["weights"])
    elif kind == "incidence_flip":
        L["exposure"] = dict(L["exposure"], incidence=not L["exposure"]["incidence"])
    elif kind == "haze_off":
        L["haze"] = None
    elif kind == "mips_off":
        L["mips"] = False
    elif kind == "mips_bias":
        L["mip_bias"] = a["mip_bias"]
    elif kind == "anisotropy":
        L["max_anisotropy"] = a["max_anisotropy"]
    elif kind == "tint_colours_only":
        for p, (hi, lo) in (("viewshed", ("visible_rgba", "hidden_rgba")), ("cumulative", ("high_rgba", "low_rgba")), ("exposure", ("high_rgba", "low_rgba"))):
            if L[p] is not None:
                L[p] = dict(L[p], **dict(zip((hi, lo), a["colours"][p])))
    elif kind == "heights_again":
        s["heights"] = a["heights"]
    return s


def chain_features(c, state):
    """the state as the features of supersample_model.chain"""
    A, D, L, Wt = state["ambient_params"], state["drape"], state["late"] or {}, state.get("water") or {}
    drape = None if D is None else dict(D, mips=bool(L.get("mips")), bias=L.get("mip_bias", 0.0), max_anisotropy=L.get("max_anisotropy", 1))
    return dict(shade_mode=c["mode"], shadows=dict(state["shadow_params"]) if state["shadows"] else None, ambient=dict(A) if state["ambient"] else None,
                drape=drape, flood=Wt.get("flood"), spill=Wt.get("spill"), exposure=L.get("exposure"), cumulative=L.get("cumulative"),
                viewshed=L.get("viewshed"), haze=L.get("haze"))


def unoccluded(c):
    """the case with no overlay layer occluding: what a supersampled handle accepts (include/vf_hip.h)"""
    return dict(c, overlays=[(kind, dict(kw, occlude=False) if "occlude" in kw else kw) for kind, kw in c["overlays"]],
                hazed=dict(c["hazed"], ladder=dict(c["hazed"]["ladder"], occlude=False)))


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
        s["overlays"], s["occlusion"], s["hazed"] = False, {}, None       # (the flags and the ladder go with the layers)
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
    follows a later exaggeration.  The layers are overlay_haze_model's: a layer the state flags (state["hazed"], with the ladder behind
    the case's own calls) takes the haze, and so does a contour layer's snapshot.  L.index: call index -> the model's layer."""
    L = ohm.Layers()
    Hz = state.get("hazed")
    flags = Hz["flags"] if Hz else {}
    L.segments = {}                                           # call index -> segments of a contour layer
    u0 = uniforms(c)
    index = {}                                                # layer id of the library -> index among the models' point / line layers
    for k, (kind, kw) in enumerate(c["overlays"]):
        if kind == "points":
            L.points(kw["xyz"], haze=bool(flags.get(k)), **{a: v for a, v in kw.items() if a != "xyz"})
        elif kind == "lines":
            L.lines(kw["paths"], haze=bool(flags.get(k)), **{a: v for a, v in kw.items() if a != "paths"})
        elif kind == "polygons":
            L.polygons(kw["polygons"], **{a: v for a, v in kw.items() if a != "polygons"})
            continue
        else:
            L.contours(c["heights"], c["grid"], u0, kw["levels"], haze=bool(flags.get(k)), **{a: v for a, v in kw.items() if a != "levels"})
            L.segments[k] = L.nsegments
        index[k] = len(L.ranges) - 1
    if Hz is not None:
        kw = c["hazed"]["ladder"]
        L.points(kw["xyz"], haze=bool(Hz["ladder"]), **{a: v for a, v in kw.items() if a != "xyz"})
        index[ladder_index(c)] = len(L.ranges) - 1
    L.index, L.counts = index, {}
    for k in index:
        a, b = L.ranges[index[k]]
        L.counts[k] = sum(len(r) for r in L.recs[a:b])
    for k, (occlude, bias) in state["occlusion"].items():
        L.set_occlusion(index[k], occlude, bias)
    return L


def expected(c, state, cache=None):
    """The reference of a handle state: the oracle's frame and visibility, then the passes in the library's order, which is written
    down once, in supersample_model.chain (the relight pass, the draped image through its mips and anisotropic taps, the flood's water,
    the spill's sink tint, the exposure, cumulative and viewshed tints, the haze), then the overlays (overlay_haze_model.composite of
    its layers under the state's haze: occlusion_model.composite's bytes without a flag or without the haze).  `cache` (a
    dict of one case) keeps the oracle's frames, the vertex fields and the results, for a caller that asks for a state twice.
    -> dict rgba (the oracle's frame), vis, shaded, mask (the pixels the shade pass writes again), draped (the frame behind the drape
    pass: `shaded` without a drape), drape_mask (the pixels the drape writes again), late (the frame behind the last late pass:
    `draped` without one), haze_opacity, stages (everything chain records), frame (what the handle must show), layers (or None)."""
    import oracle
    W, H, G, h, u = c["W"], c["H"], c["grid"], state["heights"], state["u"]
    key = (u.tobytes(), h.tobytes(), h.shape)
    A, D = state["ambient_params"], state["drape"]
    whole = (key, state["shadows"], state["ambient"], state["overlays"], tuple(sorted(state["shadow_params"].items())),
             A["strength"], A["reach"], A["directions"].tobytes(), tuple(sorted(state["occlusion"].items())),
             None if D is None else (D["image"].tobytes(), D["image"].shape, D["extent"], D["opacity"], D["filter"]), ssm._key(state["late"]),
             ssm._key(state.get("water")), None if state.get("hazed") is None else (tuple(sorted(state["hazed"]["flags"].items())), state["hazed"]["ladder"]))
    if cache is not None and whole in cache:
        return cache[whole]
    if cache is not None and key in cache:
        rgba, vis = cache[key]
    else:
        rgba, vis = oracle.render_terrain(u, W, H, G, h, lut(c["cmap"]), want_vis=True, nthreads=min(8, oracle.max_threads()), shade_mode=c["mode"])
        rgba = rgba.reshape(H, W, 4)
        if cache is not None:
            cache[key] = (rgba, vis)
    st = {}
    late = ssm.chain(rgba, vis, u, h, G, lut(c["cmap"]), stages=st, memo=cache, **chain_features(c, state))
    out = {"rgba": rgba, "vis": vis, "shaded": st["shaded"], "mask": st["mask"], "draped": st["draped"], "drape_mask": st["drape_mask"], "late": late,
           "haze_opacity": st["haze_opacity"], "stages": st, "frame": late, "layers": None}
    if state["overlays"]:
        out["layers"] = layers(c, state)
        out["frame"] = ohm.composite(late, vis, u, h, G, out["layers"], haze=the_haze(state))
    if cache is not None:
        cache[whole] = out
    return out


def expected_supersampled(c, state, f, cache=None):
    """The reference of a handle made with supersample=f in `state` (no layer occluding): the same chain at (f W, f H), the resolve,
    the overlays at (W, H) -> dict samples, vis (both at the sample size), haze_opacity, resolved, frame"""
    u, h, G = state["u"], state["heights"], c["grid"]
    st = {}
    s, vis = ssm.samples(c["W"], c["H"], f, u, h, G, lut(c["cmap"]), stages=st, memo=cache, **chain_features(c, state))
    resolved = ssm.resolve(s, f)
    L = layers(unoccluded(c), dict(state, occlusion={})) if state["overlays"] else None
    # (as supersample_model.composite: at the output size, over a zero visibility; the hazed layers under the state's haze)
    over = resolved if L is None else ohm.composite(resolved, np.zeros((c["H"], c["W"]), np.uint32), u, h, G, L, haze=the_haze(state))
    return dict(samples=s, vis=vis, haze_opacity=st["haze_opacity"], resolved=resolved, frame=over)


def the_haze(state):
    """the haze of a state as overlay_haze_model.composite takes it: set_haze's keywords, or None while the haze is off"""
    return (state.get("late") or {}).get("haze")


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


def late_shares(c, cache=None):
    """what the reference alone says about a case's late passes: on; covered (pixels); changed: per pass that is on, the share of
    the covered pixels it changes (mips: against the same drape sampled without them; None without a covered pixel, and for mips
    without a drape); field_mixed: the viewshed field has values below 0.5 and values of 1; haze_partial: an opacity strictly between
    0 and max_opacity; lod_above_0: a draped pixel samples above level 0; many_taps: a draped pixel takes more than one tap;
    covered_before_late_mutation (pixels, in the state after the case's first mutation, where run_case applies the late one);
    mutation_shows: the frame behind the late passes (under the overlays, whose draw is older and may cover anything) differs after
    the late mutation from the one before it"""
    L = c["late"]
    s1 = featured(c, initial_state(c), overlays=True)
    s2 = lated(c, s1)
    e1, e2 = expected(c, s1, cache), expected(c, s2, cache)
    st, cov = e2["stages"], e2["vis"] != 0
    covered = int(cov.sum())
    changed, before = {}, e2["draped"]
    if "mips" in L["on"]:
        changed["mips"] = int(((e2["draped"] != e1["draped"]).any(axis=2) & cov).sum()) / covered if covered and c["drape"] is not None else None
    for p in ("exposure", "cumulative", "viewshed", "haze"):
        if p in L["on"]:
            changed[p] = int(((st[p + "_frame"] != before).any(axis=2) & cov).sum()) / covered if covered else None
            before = st[p + "_frame"]
    seen = st.get("viewshed_field")
    a, smp, m = e2["haze_opacity"], st["drape_sample"], e2["drape_mask"]
    s3 = mutated(c, s2)
    e3 = expected(c, s3, cache)
    return dict(on=L["on"], supersample=L["supersample"], covered=covered, changed=changed,
                field_mixed=None if seen is None else bool((seen < 0.5).any() and (seen == 1).any()),
                haze_partial=bool(((a > 0) & (a < f32(L["haze"]["max_opacity"]))).any()) if "haze" in L["on"] else None,
                lod_above_0=None if smp is None or not m.any() else bool((smp[m][:, 6] > 0).any()),
                many_taps=None if smp is None or smp.shape[2] < 10 or not m.any() else bool((smp[m][:, 7] > 1).any()),
                covered_before_late_mutation=int((e3["vis"] != 0).sum()),
                mutation_shows=bool((expected(c, late_mutated(c, s3), cache)["late"] != e3["late"]).any()))


def describe_late(stat):
    """the late passes' shares over a list of late_shares() results, as text"""
    out = []
    for p in LATE_PASSES:
        ch = [s["changed"][p] for s in stat if s["changed"].get(p) is not None]
        out.append(f"{p} on in {sum(p in s['on'] for s in stat)} of {len(stat)}, changes a pixel in {sum(v > 0 for v in ch)} and 10-90 % in "
                   f"{sum(0.1 < v < 0.9 for v in ch)} of {len(ch)} covered")
    return "; ".join(out)


def behind_the_water(e):
    """the frame behind the spill's tint of a result of expected(): what the exposure tint, or whatever comes next, is laid over"""
    st = e["stages"]
    return st.get("spill_frame", st.get("flood_frame", e["draped"]))


def water_shares(c, cache=None):
    """what the reference alone says about a case's flood and spill: on; flood_mode; proper: the flooded set is a non-empty proper
    subset of the wet-able vertices; sinks: a vertex has a sink depth above 0; identity: flooded == reached & (spill < level) for the
    flood's own sources; covered (pixels); changed: per pass that is on, the share of the covered pixels it changes
    (None without a covered pixel); partial: a blended pixel's depth lies strictly between 0 and depth_full; covered_before_the
    mutation (pixels, in the state run_case applies it to); mutation_shows: a state the mutation leads through has another frame
    behind the water (behind_the_water) than the one before it; mutation_shows_behind_the_late_passes: the same of the frame behind
    the haze, under tints that may be opaque; without_water: the frame after it is that of the state without either pass"""
    P = c["water"]
    s2 = watered(c, lated(c, featured(c, initial_state(c), overlays=True)))
    e2 = expected(c, s2, cache)
    st, cov = e2["stages"], e2["vis"] != 0
    covered = int(cov.sum())
    surf = cm.surface(c["heights"], c["grid"])
    F = flood_of(c, surf, P["flood"])
    S = spill_of(c, surf, P["spill"])
    own = spm.field_heights(surf, _sources(c, P["flood"]["seeds"])) if P["flood"]["seeds"] is not None else None
    changed, partial, before = {}, {}, e2["draped"]
    for p, model, field in (("flood", fdm, F), ("spill", spm, S)):
        if p in P["on"]:
            changed[p] = int(((st[p + "_frame"] != before).any(axis=2) & cov).sum()) / covered if covered else None
            d = model.frame(before, e2["vis"], s2["u"], s2["heights"], c["grid"], st[p + "_field"], **{k: P[p][k] for k in ("shallow_rgba", "deep_rgba", "depth_full")})[1]
            partial[p] = bool(((d > 0) & (d < f32(P[p]["depth_full"]))).any())
            before = st[p + "_frame"]
    s3 = late_mutated(c, mutated(c, s2))
    e3 = expected(c, s3, cache)
    steps = [expected(c, s, cache) for _, s in water_steps(c, s3)]
    return dict(on=P["on"], flood_mode=flood_mode(P["flood"]), proper=bool(F.flooded.any() and (F.wet & ~F.flooded).any()), sinks=bool((S.sink > 0).any()),
                identity=None if own is None else bool(np.array_equal(F.flooded, own.reached & (own.spill < f32(P["flood"]["level"])))),
                covered=covered, changed=changed, partial=partial, covered_before_the_mutation=int((e3["vis"] != 0).sum()),
                mutation_shows=any(bool((behind_the_water(e) != behind_the_water(e3)).any()) for e in steps),
                mutation_shows_behind_the_late_passes=any(bool((e["late"] != e3["late"]).any()) for e in steps),
                without_water=bool(np.array_equal(steps[-1]["late"], expected(c, dict(water_steps(c, s3)[-1][1], water=None), cache)["late"])))


def hazed_counts(c, state, cache=None, only=None):
    """overlay_haze_model's counts over the state's reference: (the (hazed feature, covered pixel) pairs, those with 0 < S.ah <
    max_opacity, those with S.ah == 0).  `only` (a call index, or ladder_index): as if that layer alone were flagged"""
    e = expected(c, state, cache)
    L = e["layers"] if only is None else layers(c, dict(state, hazed=dict(flags={only: True}, ladder=only == ladder_index(c))))
    return ohm.composite(e["late"], e["vis"], state["u"], state["heights"], c["grid"], L, haze=the_haze(state), want_counts=True)[1]


def flagged_kinds(c):
    """what the case's flagged drawn layers are: the points' shapes, the lines' caps (cap_butt, ...), contours"""
    out = set()
    for k, on in zip(eligible(c), c["hazed"]["flags"]):
        kind, kw = c["overlays"][k]
        if on:
            out.add(kw["shape"] if kind == "points" else "cap_" + kw["cap"] if kind == "lines" else kind)
    return out


def hazed_shares(c, cache=None):
    """what the reference alone says about a case's hazed layers, in the state run_case's steps B and H meet (everything on, before
    the first mutation): haze_on; pairs, middle, clear (hazed_counts); differs: the frame is not that of the same layers unflagged;
    kinds (flagged_kinds); occluding: a flagged drawn layer occludes; early_then_add: a flag is set while layers are still to come
    (the ladder always is); mutation; covers (flag_flip: the flipped layer, flagged alone, has a covered pixel with S.ah > 0, the
    terrain in front of it taken into account); mutation_shows: a state the mutation leads through has another frame; stated
    (flags_all_off: the frame after it is occlusion_model.composite's over the same layers; polygon_refused: the frame before it)"""
    s2 = hazed_on(c, watered(c, lated(c, featured(c, initial_state(c), overlays=True))))
    e2 = expected(c, s2, cache)
    pairs, middle, clear = hazed_counts(c, s2, cache)
    kind, a = c["hazed_mutation"], c["hazed_mutation_args"]
    steps = [expected(c, s, cache) for _, s in hazed_steps(c, s2)]
    stated = None
    if kind == "flags_all_off":
        stated = bool(np.array_equal(steps[-1]["frame"], ocm.composite(e2["late"], e2["vis"], s2["u"], s2["heights"], c["grid"], e2["layers"])))
    elif kind == "polygon_refused":
        stated = bool(np.array_equal(steps[-1]["frame"], e2["frame"]))
    covers = None
    if kind == "flag_flip":
        p, _, cl = hazed_counts(c, s2, cache, only=a["layer"])
        covers = p > cl
    flagged = [k for k, on in zip(eligible(c), c["hazed"]["flags"]) if on]
    return dict(haze_on=the_haze(s2) is not None, pairs=pairs, middle=middle, clear=clear,
                differs=bool((e2["frame"] != expected(c, hazed_on(c, s2, flags=False), cache)["frame"]).any()), kinds=flagged_kinds(c),
                occluding=any(c["overlays"][k][1]["occlude"] for k in flagged),
                early_then_add=any(e for k, e in zip(eligible(c), c["hazed"]["early"]) if k in flagged), mutation=kind, covers=covers,
                mutation_shows=any(bool((e["frame"] != e2["frame"]).any()) for e in steps), stated=stated)


def describe_hazed(stat):
    """the hazed layers' shares over a list of hazed_shares() results, as text"""
    on = [s for s in stat if s["haze_on"]]
    return (f"the haze on in {len(on)} of {len(stat)}: a hazed feature covers a pixel in {sum(s['pairs'] > 0 for s in on)}, a quarter of the pairs strictly inside "
            f"in {sum(4 * s['middle'] >= s['pairs'] > 0 for s in on)}, a pair with S.ah == 0 in {sum(s['clear'] > 0 for s in on)}, the frame differs from the "
            f"unflagged one in {sum(s['differs'] for s in on)}")


def describe_water(stat):
    """the flood's and the spill's shares over a list of water_shares() results, as text"""
    out = []
    for p in WATER_PASSES:
        ch = [s["changed"][p] for s in stat if s["changed"].get(p) is not None]
        out.append(f"{p} on in {sum(p in s['on'] for s in stat)} of {len(stat)}, changes a pixel in {sum(v > 0 for v in ch)} and 10-90 % in "
                   f"{sum(0.1 < v < 0.9 for v in ch)} of {len(ch)} covered")
    listed = [s for s in stat if "flood" in s["on"] and s["flood_mode"] != "everywhere"]
    spilt = [s for s in stat if "spill" in s["on"]]
    out.append(f"the flooded set is a proper non-empty subset of the wet-able vertices in {sum(s['proper'] for s in listed)} of {len(listed)} floods from edges or seeds, "
               f"sinks in {sum(s['sinks'] for s in spilt)} of {len(spilt)} spills")
    return "; ".join(out)


# ---- the GPU side ----------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _where(d):
    return int(d.sum()), np.argwhere(d)[:4].tolist()


def _add_overlays(t, c, hazed=None, swap=False):
    """the case's overlay calls on the handle -> (layer ids, contour segment counts by call index).  `hazed` (a state's entry): the
    ladder is added behind them, and the flags are set as the case's `early` says -- `swap`: the other way round -- directly after
    the layer's add (the side array is allocated at the record array's capacity of that moment and grows with every later append,
    a contour layer's GPU-extracted records among them) or after all adds"""
    ids, nseg, late = {}, {}, []
    early = dict(zip(eligible(c), c["hazed"]["early"])) if hazed is not None else {}
    for k, (kind, kw) in enumerate(list(c["overlays"]) + ([("points", c["hazed"]["ladder"])] if hazed is not None else [])):
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
        if hazed is not None and (hazed["ladder"] if k == ladder_index(c) else hazed["flags"].get(k)):
            if k != ladder_index(c) and early[k] != swap:
                t.set_layer_haze(ids[k], True)
            else:
                late.append(k)
    for k in late:
        t.set_layer_haze(ids[k], True)
    return ids, nseg


def _flags_differ(t, c, state, ids):
    """layer_haze() of every layer of the handle against the state's flags (a polygon layer: never) -> the layers that differ"""
    Hz = state["hazed"]
    want = {k: bool(Hz["ladder"] if k == ladder_index(c) else Hz["flags"].get(k, False)) for k in ids}
    return [k for k in ids if t.layer_haze(ids[k]) is not want[k]]


def _refused(call, message):
    """whether `call` raises with `message` (vf_last_error's text)"""
    try:
        call()
    except RuntimeError as e:
        return message in str(e)
    return False


def _apply_hazed_mutation(t, c, after, ids, wrong):
    """one step of the hazed mutation on the handle -> the layer ids then"""
    kind, a = c["hazed_mutation"], c["hazed_mutation_args"]
    if kind == "flag_flip":
        t.set_layer_haze(ids[a["layer"]], after["hazed"]["flags"][a["layer"]])
    elif kind == "flags_all_off":
        for k in ids:
            if k == ladder_index(c) or k in after["hazed"]["flags"]:
                t.set_layer_haze(ids[k], False)
    elif kind == "haze_params":
        _set_late(t, c, after)
    elif kind == "occlusion_on_hazed":
        t.set_layer_occlusion(ids[a["occlusion_layer"]], *after["occlusion"][a["occlusion_layer"]])
    elif kind == "readd":
        t.clear_overlays()                                    # (with flags set the first time, with none the second)
        for k in ids:
            if not _refused(lambda: t.layer_haze(ids[k]), UNKNOWN_LAYER):
                wrong(f"layer_haze({ids[k]}) after clear_overlays is not refused with '{UNKNOWN_LAYER}'")
        ids, _ = _add_overlays(t, c, after["hazed"], swap=True)
    elif kind == "polygon_refused":
        polygon = next(k for k, (kind_, _) in enumerate(c["overlays"]) if kind_ == "polygons")
        if not _refused(lambda: t.set_layer_haze(ids[polygon], True), POLYGON_REFUSED):
            wrong(f"set_layer_haze on the polygon layer {ids[polygon]} is not refused with '{POLYGON_REFUSED}'")
        if not _refused(lambda: t.set_layer_haze(len(ids), True), UNKNOWN_LAYER):
            wrong(f"set_layer_haze on the unknown layer {len(ids)} is not refused with '{UNKNOWN_LAYER}'")
    return ids


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
        state = hazed_on(c, dict(state, overlays=True))       # (the haze is not on yet: the flags and the ladder, the unflagged bytes)
        ids, nseg = _add_overlays(t, c, state["hazed"])
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
        if _flags_differ(t, c, state, ids):
            bad.append((seed, 4, f"layer_haze() of the layers {_flags_differ(t, c, state, ids)} against the flags set", 1, []))
        compare_planes(4, state, e["vis"])                    # (the planes and the visibility know nothing of the drape)
        differ(4, "visibility", t.read_visibility() != e["vis"])
        # A. the late passes' vertex fields: their parameters set, the passes off
        P, u, h, lut_ = c["late"], state["u"], state["heights"], lut(c["cmap"])
        _set_late(t, c, state)
        V, M, X = P["viewshed"], P["cumulative"], P["exposure"]
        seen, vtx = vsm.field(u, h, G, V["observer"], **{k: V[k] for k in _SCAN})
        differ("A", "viewshed field", _bits(t.viewshed_field()) != _bits(seen))
        info, n = t.viewshed_info(), max(G, 2)
        with np.errstate(invalid="ignore"):
            xyz = (vertex_xz(vtx[0], vtx[1], n, c["spacing"])[0], float(shm.heights(u, h, G)[vtx[1], vtx[0]] * u[38]), vertex_xz(vtx[0], vtx[1], n, c["spacing"])[1])
        # (the position has no bit-exact statement in the contract: the model's vertex, and its place to a few binary32 steps)
        if info["vertex"] != tuple(vtx) or not np.allclose(info["observer_xyz"], xyz, rtol=1e-5, atol=1e-6, equal_nan=True):
            bad.append((seed, "A", f"viewshed_info() vertex {info['vertex']} at {info['observer_xyz']} against {tuple(vtx)} at {xyz}", 1, []))
        cnt, verts = cvm.field(u, h, G, M["observers"], radius=M["radius"], **{k: M[k] for k in _SCAN})
        differ("A", "cumulative viewshed field", _bits(t.cumulative_viewshed_field()) != _bits(cnt))
        if t.cumulative_viewshed_info()["vertices"].tolist() != [list(v) for v in verts]:
            bad.append((seed, "A", "cumulative_viewshed_info() vertices against the model's", 1, []))
        t.cumulative_viewshed_batch(M["batch"])
        differ("A", f"cumulative viewshed field at batch size {M['batch']}", _bits(t.cumulative_viewshed_field()) != _bits(cnt))
        expo = sem.field(u, h, G, X["suns"], X["weights"], incidence=X["incidence"], softness=X["softness"], bias=X["bias"])
        differ("A", "sun exposure field", _bits(t.sun_exposure_field()) != _bits(expo))
        t.sun_exposure_batch(X["batch"])
        differ("A", f"sun exposure field at batch size {X['batch']}", _bits(t.sun_exposure_field()) != _bits(expo))
        _water_fields(t, c, state, differ, lambda what: bad.append((seed, "A", what, 1, [])))
        # B. the late passes and the water on, exact precision, the overlays still on; the second frame is the one planned ahead
        state = watered(c, lated(c, state))
        _set_late(t, c, state)
        _set_water(t, c, state)
        e = expected(c, state, cache)
        for again in ("", " drawn again"):
            differ("B", "frame" + again, (frame(t) != e["frame"]).any(axis=2))
        # (the opacity plane follows the stored settings, enabled or not)
        differ("B", "haze opacity", _bits(t.haze_opacity()) != _bits(hzm.frame(e["late"], e["vis"], u, h, G, **P["haze"])[1]))
        info, D = t.drape_mip_info(), state["drape"]
        if not state["late"]["mips"]:
            if info is not None:
                bad.append((seed, "B", f"drape_mip_info() {info} with mipmaps off", 1, []))
        else:
            sz = [] if D is None else dmm.sizes(D["image"].shape[1], D["image"].shape[0])
            if info is None or info["levels"] != len(sz) or [tuple(s) for s in info["sizes"]] != sz or info["builds"] != int(len(sz) >= 2):
                bad.append((seed, "B", f"drape_mip_info() {info} against the sizes {sz} and {int(len(sz) >= 2)} builds", 1, []))
            elif len(sz) >= 2:
                k = 1 + zlib.crc32(c["name"].encode()) % (len(sz) - 1)
                differ("B", f"pyramid level {k}", (t.read_drape_level(k).view(np.uint16) != dmm.pyramid(D["image"])[k].view(np.uint16)).any(axis=2))
        # C. fast precision.  The fast frame before the late passes is known without reading it: the relit and draped pixels are the
        # exact ones (with mips and anisotropy on, that is asserted here for the first time) and every other pixel is the plain fast
        # frame's.  The tints and the haze do not follow the precision, so off the pixels an overlay touches the frame is their
        # models' over that frame, bit for bit, written pixels and others alike
        t.set_shade_precision(1)
        got = frame(t)
        before = np.where((e["mask"] | e["drape_mask"])[..., None], e["draped"], plain)
        want = ssm.chain(before, e["vis"], u, h, G, lut_, memo=cache, **dict(chain_features(c, state), shadows=None, ambient=None, drape=None))
        touched = ((ohm.composite(want, e["vis"], u, h, G, e["layers"], haze=the_haze(state)) != want)
                   | (ohm.composite(255 - want, e["vis"], u, h, G, e["layers"], haze=the_haze(state)) != 255 - want)).any(axis=2)
        differ("C", "fast frame off the overlays against the late passes' models over the fast frame before them", (got != want).any(axis=2) & ~touched)
        differ("C", "fast frame's alpha", got[..., 3] != e["frame"][..., 3])
        t.set_shade_precision(0)
        # H. the hazed mutation, while everything is on: the frame, layer_haze() of every layer and, for polygon_refused, the messages
        kind = c["hazed_mutation"]
        for what, after in hazed_steps(c, state):
            ids = _apply_hazed_mutation(t, c, after, ids, lambda text: bad.append((seed, "H", text, 1, [])))
            state = after
            differ("H", f"frame after {kind}: {what}", (frame(t) != expected(c, state, cache)["frame"]).any(axis=2))
            if _flags_differ(t, c, state, ids):
                bad.append((seed, "H", f"after {kind} ({what}): layer_haze() of the layers {_flags_differ(t, c, state, ids)} against the flags set", 1, []))
        # D (and 5). the mutation, then the late mutation
        kind, a = c["mutation"], c["mutation_args"]
        scans, late_scans = (t.shadow_scans(), t.ambient_scans()), _late_counters(t)
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
        late_scans = _late_stale(bad, seed, 5, kind, t, state, late_scans)
        before = state
        kind = c["late_mutation"]
        state = late_mutated(c, state)
        _apply_late_mutation(t, c, state)
        differ("D", f"frame after {kind}", (frame(t) != expected(c, state, cache)["frame"]).any(axis=2))
        late_scans = _late_stale(bad, seed, "D", kind, t, state, late_scans, _reordered(c, before, state))
        # W. the water mutation
        kind = c["water_mutation"]
        for what, after in water_steps(c, state):
            before, state = state, after
            _apply_water_mutation(t, c, state)
            differ("W", f"frame after {kind}: {what}", (frame(t) != expected(c, state, cache)["frame"]).any(axis=2))
        _late_stale(bad, seed, "W", kind, t, state, late_scans, moved=_seeds_moved(c, before, state))
        # 6. the drape cleared: the frame of the same state without one
        if state["drape"] is not None:
            state = dict(state, drape=None)
            _set_drape(t, None)
            differ(6, "frame after clear_drape", (frame(t) != expected(c, state, cache)["frame"]).any(axis=2))
        if t.drape_info() is not None:
            bad.append((seed, 6, f"drape_info() {t.drape_info()} after clear_drape", 1, []))
    finally:
        t.close()
    # E. a supersampled second handle: the same heights, uniforms, features, drape and late passes, no layer occluding; then the late mutation
    f = c["late"]["supersample"]
    if f > 1:
        state = hazed_on(c, watered(c, lated(c, featured(c, initial_state(c), overlays=True))))
        t = cabi.Terrain(W, H, G, lut(c["cmap"]), supersample=f)
        try:
            t.set_uniforms(state["u"]); t.set_shade_mode(c["mode"]); t.set_height(state["heights"]); t.set_shade_precision(0)
            _set_features(t, state)
            _set_drape(t, state["drape"])
            _set_late(t, c, state)
            _set_water(t, c, state)
            _add_overlays(t, unoccluded(c), state["hazed"])       # (the flags and the ladder, none occluding)
            for step in ("E", "E after " + c["late_mutation"], "E after " + c["water_mutation"]):
                if step == "E after " + c["late_mutation"]:
                    state = late_mutated(c, state)
                    _apply_late_mutation(t, c, state)
                elif step != "E":
                    for _, state in water_steps(c, state):
                        _apply_water_mutation(t, c, state)
                e = expected_supersampled(c, state, f, cache)
                t.render()
                differ(step, "samples", (t.read_samples() != e["samples"]).any(axis=2))
                differ(step, "frame against the resolve and the overlays", (t.read_rgba().reshape(H, W, 4) != e["frame"]).any(axis=2))
                differ(step, "visibility of the samples", t.read_visibility() != e["vis"])
        finally:
            t.close()
    return bad


_SCAN = ("eye_height", "target_height", "softness", "bias")


def _set_late(t, c, state):
    """The late passes' settings on the handle, all of them by every call (a setting sent again as it stands must cost nothing): a
    pass is on where the state has it, with the state's parameters; an off pass keeps the case's"""
    P, L = c["late"], state["late"] or {}
    t.set_drape_mipmaps(bool(L.get("mips")), bias=L.get("mip_bias", P["mip_bias"]))
    t.set_drape_anisotropy(L.get("max_anisotropy", P["max_anisotropy"]))
    V, M, X, Z = (L.get(p) or P[p] for p in LATE_PASSES[1:])
    t.set_viewshed(V["observer"], enabled=L.get("viewshed") is not None, radius=V["radius"], visible_rgba=V["visible_rgba"], hidden_rgba=V["hidden_rgba"],
                   **{k: V[k] for k in _SCAN})
    t.set_cumulative_viewshed(M["observers"], enabled=L.get("cumulative") is not None, radius=M["radius"], high_rgba=M["high_rgba"], low_rgba=M["low_rgba"],
                              **{k: M[k] for k in _SCAN})
    t.set_sun_exposure(X["suns"], weights=X["weights"], incidence=X["incidence"], enabled=L.get("exposure") is not None, softness=X["softness"], bias=X["bias"],
                       high_rgba=X["high_rgba"], low_rgba=X["low_rgba"])
    t.set_haze(Z["density"], enabled=L.get("haze") is not None, **{k: Z[k] for k in ("rgba", "start", "falloff", "base", "max_opacity", "background")})


def _apply_late_mutation(t, c, state):
    """the late mutation's state on the handle"""
    if c["late_mutation"] == "heights_again":
        t.set_height(state["heights"])
    else:
        _set_late(t, c, state)


def _set_water(t, c, state):
    """The flood's and the spill's settings on the handle, all of them by every call: a pass is on where the state has it, with the
    state's parameters; an off pass keeps the case's; a cleared spill is cleared"""
    P, Wt = c["water"], state.get("water") or {}
    F, S = Wt.get("flood") or P["flood"], Wt.get("spill") or P["spill"]
    t.set_flood(F["level"], F["seeds"], enabled=Wt.get("flood") is not None, shallow_rgba=F["shallow_rgba"], deep_rgba=F["deep_rgba"], depth_full=F["depth_full"])
    if Wt.get("cleared"):
        t.clear_spill()
    else:
        t.set_spill(S["seeds"], enabled=Wt.get("spill") is not None, shallow_rgba=S["shallow_rgba"], deep_rgba=S["deep_rgba"], depth_full=S["depth_full"])


def _apply_water_mutation(t, c, state):
    """the water mutation's state on the handle"""
    if c["water_mutation"] == "heights_water":
        t.set_height(state["heights"])
    else:
        _set_water(t, c, state)


def _seeds_moved(c, before, after):
    """per pass: whether the list of its seeds' vertices reads differently (what the field's key holds of them)"""
    def vertices(P):
        return None if P is None or not isinstance(P["seeds"], np.ndarray) else seed_vertices(c, P["seeds"]).tolist()
    return {p: vertices(before["water"][p]) != vertices(after["water"][p]) for p in WATER_PASSES}


def _water_fields(t, c, state, differ, wrong):
    """Step A of the water: both passes set and off; the three fields against the models bit for bit, flood_info() and spill_info()
    against the models' counts, modes and vertices, the passes and tile runs inside the bounds of tests/test_gpu_flood.py and
    tests/test_gpu_spill.py against the models' tile_passes (the kernels may see a neighbour's stores of the same launch, so they never
    need more passes than the emulation with halos from before the pass; a pass that changes something is followed by another);
    then each field read again at the case's other group size: the same bits, one more scan for a new group size"""
    P, u, h, G = c["water"], state["u"], state["heights"], c["grid"]
    _set_water(t, c, state)
    tiles = spm.n_tiles(max(G, 2))
    surf = cm.surface(h, G)
    F = fdm.field(u, h, G, P["flood"]["level"], P["flood"]["seeds"])
    S = spm.field(u, h, G, P["spill"]["seeds"])
    flooded, emulated = fdm.tile_passes(F.wet, fdm.sources(F.wet, "edges" if isinstance(P["flood"]["seeds"], str) else F.vertices)) if P["flood"]["seeds"] is not None else (F.flooded, 0)
    if not np.array_equal(flooded, F.flooded):
        wrong("the flood model's tile passes against its search")
    S2, spill_emulated, _ = spm.tile_passes(surf, "edges" if isinstance(P["spill"]["seeds"], str) else S.vertices)
    if (_bits(S2.spill) != _bits(S.spill)).any():
        wrong("the spill model's tile passes against its search")

    def vertices_differ(info, M):
        return (info["vertices"] is not None or info["seeds"] != 0) if M.vertices is None else not (info["vertices"] is not None and np.array_equal(info["vertices"], M.vertices))

    def flood(what):
        differ("A", "flood field" + what, _bits(t.flood_field()) != _bits(F.depth))
        info = t.flood_info()
        if (info["flooded_vertices"], info["wettable_vertices"], info["mode"]) != (int(F.flooded.sum()), int(F.wet.sum()), flood_mode(P["flood"])) or vertices_differ(info, F):
            wrong(f"flood_info(){what} {info} against {int(F.flooded.sum())} flooded of {int(F.wet.sum())} wet-able, {flood_mode(P['flood'])}, the model's vertices")
        if not (min(emulated, 2) <= info["passes"] <= emulated) or info["level"] != float(f32(P["flood"]["level"])):
            wrong(f"flood_info(){what}: {info['passes']} passes against the emulation's {emulated}, level {info['level']}")
        return info

    def spill(what, flags=True):
        differ("A", "spill field" + what, _bits(t.spill_field()) != _bits(S.spill))
        differ("A", "sink depth field" + what, _bits(t.sink_depth_field()) != _bits(S.sink))
        info = t.spill_info()
        if (info["reached_vertices"], info["sink_vertices"], info["mode"]) != (int(S.reached.sum()), int((S.sink > 0).sum()), spill_mode(P["spill"])) or vertices_differ(info, S):
            wrong(f"spill_info(){what} {info} against {int(S.reached.sum())} reached, {int((S.sink > 0).sum())} sinks, {spill_mode(P['spill'])}, the model's vertices")
        queued = -(-info["passes"] // max(info["group"], 1)) * info["group"]      # (the passes of the last group behind the fixpoint run too)
        runs_ok = info["tile_runs"] <= info["passes"] * tiles and (info["tile_runs"] >= 1 or not S.reached.any()) if flags else info["tile_runs"] == queued * tiles
        if not (min(spill_emulated, 2) <= info["passes"] <= spill_emulated) or not runs_ok:
            wrong(f"spill_info(){what}: {info['passes']} passes against the emulation's {spill_emulated}, {info['tile_runs']} tile runs of {tiles} tiles, group {info['group']}")
        return info

    a, b = flood(""), spill("")
    t.flood_group(P["flood_group"])
    t.spill_group(P["spill_group"], flags=P["spill_flags"])
    a2, b2 = flood(f" at group size {P['flood_group']}"), spill(f" at group size {P['spill_group']}, flags {P['spill_flags']}", P["spill_flags"])
    rose, must = (a2["scans"] - a["scans"], b2["scans"] - b["scans"]), (int(P["flood_group"] != 0), int(P["spill_group"] != 0 or not P["spill_flags"]))
    if rose != must or (P["flood_group"] and a2["group"] != P["flood_group"]) or (P["spill_group"] and b2["group"] != P["spill_group"]):
        wrong(f"the flood / spill field was computed {rose} times for the group sizes {P['flood_group']} / {P['spill_group']}, flags {P['spill_flags']}: {must} expected")


def _late_counters(t):
    """(viewshed, cumulative, exposure, flood, spill scans, pyramid builds) over the handle's life; the builds also while mipmaps are off"""
    return (t.viewshed_scans(), t.cumulative_viewshed_scans(), t.sun_exposure_scans(), t.flood_scans(), t.spill_scans(), t.drape_mip_builds())


def _reordered(c, before, after):
    """whether the list of the cumulative observers' vertices reads differently: what the field's key holds of them"""
    a, b = before["late"]["cumulative"], after["late"]["cumulative"]
    return a is not None and [snap(c, o) for o in a["observers"]] != [snap(c, o) for o in b["observers"]]


def _late_stale(bad, seed, step, kind, t, state, counters, reordered=True, moved=None):
    """after mutation `kind` and a frame: the three late vertex fields, the flood and spill fields and the pyramid were computed as
    often as the contract says (STALE_VIEWSHED, ...: of a pass that is on) -> the counters now"""
    L, D, Wt = state["late"], state["drape"], state["water"]
    now = _late_counters(t)
    rose = tuple(int(a - b) for a, b in zip(now, counters))
    levels = 0 if D is None else len(dmm.sizes(D["image"].shape[1], D["image"].shape[0]))
    must = (int(L["viewshed"] is not None and kind in STALE_VIEWSHED),
            int(L["cumulative"] is not None and kind in STALE_CUMULATIVE and (kind != "cumulative_reorder" or reordered)),
            int(L["exposure"] is not None and kind in STALE_EXPOSURE),
            int(Wt["flood"] is not None and kind in STALE_FLOOD and (kind != "seeds_move" or moved["flood"])),
            int(Wt["spill"] is not None and kind in STALE_SPILL and (kind != "seeds_move" or moved["spill"])),
            int(L["mips"] and kind in MIP_BUILDS and levels >= 2))
    if rose != must:
        bad.append((seed, step, f"after {kind} the viewshed / cumulative / exposure / flood / spill field and the pyramid were computed {rose} times, the contract says {must}", 1, []))
    return now


FRESH_SEED = 50000                                            # the script's default window: apart from the suite's (test_gpu_feature_soak.py)
MAX_SKIPPED = 0.1                                             # the share of the seeds that may be skipped for a degenerate camera


def run(first=FRESH_SEED, cases=200, budget=400.0, verbose=True, corners=True):
    """CORNERS first (unless `corners` is false: the suite runs them as tests of their own), then seeds first .. first + cases - 1
    (until `budget` seconds have passed) -> dict: cases (seeds done), corners (done), skipped (seeds with a degenerate camera), bad
    (the tuples of run_case), summary."""
    t0 = time.time()
    say = (lambda *a: print(*a, flush=True)) if verbose else (lambda *a: None)
    bad, done, skipped, stat, late, water, hazed = [], 0, 0, [], [], [], []

    def one(c, seed):
        cache = {}
        stat.append(shares(c, cache))
        late.append(late_shares(c, cache))
        water.append(water_shares(c, cache))
        hazed.append(hazed_shares(c, cache))
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
               f"bound {100.0 * MAX_SKIPPED:.0f} %): {len(bad)} mismatches; {describe(stat)}; the late passes: {describe_late(late)}, supersampled {sum(c['supersample'] > 1 for c in late)}; the water: {describe_water(water)}; the hazed layers: {describe_hazed(hazed)}; {time.time() - t0:.0f} s")
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
