"""Argument rules of the overlay methods (Scene / TerrainSpike .add_points / .add_lines / .add_polygons / .add_contours /
.set_layer_occlusion / .set_layer_haze), pack_lines and pack_polygons.

The extension calls these before it hands the arrays to the C-ABI (include/vf_hip.h, overlays); they need numpy only, no device.
"""
from __future__ import annotations

import numbers

import numpy as np

SHAPES = {"circle": 0, "square": 1}
CAPS = {"butt": 0, "square": 1, "round": 2}
JOINS = {"round": 0, "none": 1}
MAX_CONTOUR_LEVELS = 65536                                    # include/vf_hip.h, vf_terrain_add_contours


def _float_array(obj, what):
    a = obj if isinstance(obj, np.ndarray) else np.asarray(obj)
    if a.dtype not in (np.float32, np.float64):
        raise TypeError(f"{what} must be a float32 or float64 array, got dtype {a.dtype}")
    return a


def _xyz(obj, what):
    a = _float_array(obj, what)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{what} must have shape (N, 3), got {a.shape}")
    return np.ascontiguousarray(a, dtype=np.float32)


def _colour(rgba, n, per_feature):
    """(default 4 bytes, per-feature (n, 4) uint8 array or None)"""
    if isinstance(rgba, np.ndarray) and rgba.ndim == 2:
        if not per_feature:
            raise ValueError("rgba must be a 4-tuple of ints 0-255 for a line layer")
        if rgba.dtype != np.uint8:
            raise TypeError(f"rgba as an array must be uint8, got dtype {rgba.dtype}")
        if rgba.shape != (n, 4):
            raise ValueError(f"rgba must have shape ({n}, 4), got {rgba.shape}")
        return np.zeros(4, np.uint8), np.ascontiguousarray(rgba)
    try:
        vals = tuple(rgba)
    except TypeError:
        raise TypeError("rgba must be a 4-tuple of ints 0-255" + (" or an (N, 4) uint8 array" if per_feature else "")) from None
    if len(vals) != 4:
        raise ValueError(f"rgba must hold 4 values (r, g, b, alpha), got {len(vals)}")
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError(f"rgba values must be ints 0-255, got {v!r}")
        if not 0 <= int(v) <= 255:
            raise ValueError(f"rgba values must be in 0..255, got {int(v)}")
    return np.array([int(v) for v in vals], np.uint8), None


def _size(value, n, what):
    """(default size, per-feature (n,) float32 array or None)"""
    if isinstance(value, numbers.Real) and not isinstance(value, bool):
        v = float(value)
        if not np.isfinite(v) or v <= 0.0:
            raise ValueError(f"{what} must be a positive finite number, got {v}")
        return v, None
    a = _float_array(value, what)
    if a.shape != (n,):
        raise ValueError(f"{what} must be a float or an array of shape ({n},), got shape {a.shape}")
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError(f"{what} values must be positive and finite")
    return 0.0, np.ascontiguousarray(a, dtype=np.float32)


def point_args(xyz, size_px, rgba, shape):
    """-> (xyz (N, 3) f32, default size, sizes (N,) f32 or None, default rgba (4,) u8, rgba (N, 4) u8 or None, shape code)"""
    if shape not in SHAPES:
        raise ValueError(f"shape must be one of {sorted(SHAPES)}, got {shape!r}")
    pts = _xyz(xyz, "xyz")
    n = pts.shape[0]
    dsize, sizes = _size(size_px, n, "size_px")
    dcol, cols = _colour(rgba, n, True)
    return pts, dsize, sizes, dcol, cols, SHAPES[shape]


def occlusion_args(occlude, depth_bias):
    """-> (occlude, depth_bias as a float) for add_points / add_lines / set_layer_occlusion"""
    if not isinstance(occlude, (bool, np.bool_)):
        raise TypeError(f"occlude must be a bool, got {type(occlude).__name__}")
    if isinstance(depth_bias, bool) or not isinstance(depth_bias, numbers.Real):
        raise TypeError(f"depth_bias must be a number, got {type(depth_bias).__name__}")
    b = float(depth_bias)
    if not np.isfinite(b) or b < 0.0 or b > float(np.finfo(np.float32).max):
        raise ValueError(f"depth_bias must be a finite number >= 0, got {b}")
    return bool(occlude), b


def haze_arg(haze, what="haze"):
    """-> haze as a bool, for add_points / add_lines / add_contours (haze=) and set_layer_haze (on=)"""
    if not isinstance(haze, (bool, np.bool_)):
        raise TypeError(f"{what} must be a bool, got {type(haze).__name__}")
    return bool(haze)


def pack_lines(paths):
    """Paths (a sequence of (k, 3) float arrays) -> (coords (M, 3) float32, offsets (P + 1,) uint32), consecutive duplicate vertices
    removed (ROADMAP V3.1).  A path with fewer than 2 distinct consecutive vertices, or with a non-finite coordinate, is refused."""
    if isinstance(paths, np.ndarray):
        paths = [paths] if paths.ndim == 2 else list(paths)
    out, offsets = [], [0]
    for k, p in enumerate(paths):
        a = _xyz(p, f"path {k}")
        if not np.isfinite(a).all():
            raise ValueError(f"path {k} has a non-finite coordinate")
        if len(a) > 1:
            keep = np.ones(len(a), bool)
            keep[1:] = (a[1:] != a[:-1]).any(axis=1)
            a = a[keep]
        if len(a) < 2:
            raise ValueError(f"path {k} has fewer than 2 points (after removing consecutive duplicates)")
        out.append(a)
        offsets.append(offsets[-1] + len(a))
    coords = np.concatenate(out) if out else np.zeros((0, 3), np.float32)
    return np.ascontiguousarray(coords, dtype=np.float32), np.asarray(offsets, dtype=np.uint32)


def line_args(paths, width_px, rgba, cap):
    """-> (coords (M, 3) f32, offsets (P + 1,) u32, width, rgba (4,) u8, cap code)"""
    if cap not in CAPS:
        raise ValueError(f"cap must be one of {sorted(CAPS)}, got {cap!r}")
    if isinstance(width_px, bool) or not isinstance(width_px, numbers.Real):
        raise TypeError(f"width_px must be a number, got {type(width_px).__name__}")
    width, _ = _size(width_px, 0, "width_px")
    dcol, _ = _colour(rgba, 0, False)
    coords, offsets = pack_lines(paths)
    return coords, offsets, width, dcol, CAPS[cap]


def _ring(a, f, r):
    """one ring -> (k, 3) float32 with consecutive duplicates and a closing vertex equal to the first removed"""
    a = _xyz(a, f"polygon {f} ring {r}")
    if not np.isfinite(a).all():
        raise ValueError(f"polygon {f} ring {r} has a non-finite coordinate")
    if len(a) > 1:
        keep = np.ones(len(a), bool)
        keep[1:] = (a[1:] != a[:-1]).any(axis=1)
        a = a[keep]
    if len(a) > 1 and (a[-1] == a[0]).all():
        a = a[:-1]
    if len(np.unique(a, axis=0)) < 3:
        raise ValueError(f"polygon {f} ring {r} has fewer than 3 distinct vertices (after removing duplicates and the closing vertex)")
    return a


def pack_polygons(polygons):
    """Polygons -> (coords (M, 3) float32, ring_offsets (R + 1,) uint32, feature_offsets (F + 1,) uint32).

    A polygon is one (k, 3) ring array or a sequence of rings: exteriors and holes in any number and orientation (the fill rule is
    even-odd), so a MultiPolygon is one polygon.  Consecutive duplicate vertices are removed, and so is a closing vertex equal to the
    first (rings close by themselves).  A ring with fewer than 3 distinct vertices, or with a non-finite coordinate, is refused."""
    if isinstance(polygons, np.ndarray):
        polygons = [polygons] if polygons.ndim == 2 else list(polygons)
    out, rings, feats = [], [0], [0]
    for f, poly in enumerate(polygons):
        ring_list = [poly] if isinstance(poly, np.ndarray) and poly.ndim == 2 else list(poly)
        if not ring_list:
            raise ValueError(f"polygon {f} has no ring")
        for r, ring in enumerate(ring_list):
            a = _ring(ring, f, r)
            out.append(a)
            rings.append(rings[-1] + len(a))
        feats.append(len(rings) - 1)
    coords = np.concatenate(out) if out else np.zeros((0, 3), np.float32)
    return (np.ascontiguousarray(coords, dtype=np.float32), np.asarray(rings, dtype=np.uint32), np.asarray(feats, dtype=np.uint32))


def polygon_args(polygons, fill_rgba, line_rgba, line_width_px):
    """-> (coords, ring_offsets, feature_offsets, default fill (4,) u8 or None, fills (F, 4) u8 or None, line rgba (4,) u8 or None,
    line width)"""
    if fill_rgba is None and line_rgba is None:
        raise ValueError("fill_rgba and line_rgba cannot both be None: a polygon layer needs a fill, an outline or both")
    if isinstance(line_width_px, bool) or not isinstance(line_width_px, numbers.Real):
        raise TypeError(f"line_width_px must be a number, got {type(line_width_px).__name__}")
    width, _ = _size(line_width_px, 0, "line_width_px")
    coords, rings, feats = pack_polygons(polygons)
    dfill = fills = line = None
    if fill_rgba is not None:
        dfill, fills = _colour(fill_rgba, len(feats) - 1, True)
        if fills is not None:
            dfill = None
    if line_rgba is not None:
        line, _ = _colour(line_rgba, 0, False)
    return coords, rings, feats, dfill, fills, line, width


def contour_args(levels, interval, base, width_px, rgba, lift, join, bounds=None):
    """-> (levels (K,) f32 ascending, width, rgba (4,) u8, lift, join code) for add_contours.

    Exactly one of `levels` (a 1-D float array, finite, strictly ascending, 1 .. 65536 values) and `interval` (> 0).  With `interval`
    the levels are float32(base + k * interval) for every integer k whose level lies within `bounds` = (lo, hi), the handle's
    height_bounds(): formed in float64 and rounded once."""
    if (levels is None) == (interval is None):
        raise ValueError("add_contours needs exactly one of levels and interval")
    if join not in JOINS:
        raise ValueError(f"join must be one of {sorted(JOINS)}, got {join!r}")
    if isinstance(width_px, bool) or not isinstance(width_px, numbers.Real):
        raise TypeError(f"width_px must be a number, got {type(width_px).__name__}")
    width, _ = _size(width_px, 0, "width_px")
    col, _ = _colour(rgba, 0, False)
    if isinstance(lift, bool) or not isinstance(lift, numbers.Real):
        raise TypeError(f"lift must be a number, got {type(lift).__name__}")
    lift = float(lift)
    if not np.isfinite(lift) or abs(lift) > float(np.finfo(np.float32).max):
        raise ValueError(f"lift must be a finite number, got {lift}")
    if levels is not None:
        lv = _float_array(levels, "levels")
        if lv.ndim != 1:
            raise ValueError(f"levels must be a 1-D array, got shape {lv.shape}")
        if not 1 <= lv.size <= MAX_CONTOUR_LEVELS:
            raise ValueError(f"levels must hold 1 .. {MAX_CONTOUR_LEVELS} values, got {lv.size}")
        if not np.isfinite(lv).all():
            raise ValueError("levels must be finite")
        with np.errstate(over="ignore"):
            lv = np.ascontiguousarray(lv, dtype=np.float32)
        if not np.isfinite(lv).all():
            raise ValueError("levels must be finite as float32")
        if not (lv[1:] > lv[:-1]).all():
            raise ValueError("levels must be strictly ascending (as float32)")
        return lv, width, col, lift, JOINS[join]
    for name, v in (("interval", interval), ("base", base)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise TypeError(f"{name} must be a number, got {type(v).__name__}")
    interval, base = float(interval), float(base)
    if not np.isfinite(interval) or interval <= 0.0:
        raise ValueError(f"interval must be a positive finite number, got {interval}")
    if not np.isfinite(base):
        raise ValueError(f"base must be a finite number, got {base}")
    if bounds is None:
        raise ValueError("interval needs the height bounds of the surface")
    lo, hi = float(bounds[0]), float(bounds[1])
    if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
        raise ValueError("the surface has no finite height: no contour levels")
    k0, k1 = np.ceil((lo - base) / interval) - 1.0, np.floor((hi - base) / interval) + 1.0
    if k1 - k0 + 1.0 > MAX_CONTOUR_LEVELS + 2:
        raise ValueError(f"interval {interval} gives more than {MAX_CONTOUR_LEVELS} levels over the height bounds [{lo}, {hi}]")
    lv = (base + np.arange(int(k0), int(k1) + 1, dtype=np.float64) * interval).astype(np.float32)
    lv = lv[(lv >= np.float32(lo)) & (lv <= np.float32(hi))]
    if lv.size > MAX_CONTOUR_LEVELS:
        raise ValueError(f"interval {interval} gives more than {MAX_CONTOUR_LEVELS} levels over the height bounds [{lo}, {hi}]")
    if lv.size == 0:
        raise ValueError(f"no level base + k * interval lies within the height bounds [{lo}, {hi}]")
    if not (lv[1:] > lv[:-1]).all():
        raise ValueError(f"interval {interval} is too small: consecutive levels round to the same float32")
    return np.ascontiguousarray(lv), width, col, lift, JOINS[join]
