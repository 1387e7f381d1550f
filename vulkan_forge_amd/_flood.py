"""Argument rules of the flood methods (Scene / TerrainSpike .set_flood / .flood_info).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, flood analysis); they need no device.
"""
from __future__ import annotations

import numpy as np

from ._shadows import _number
from ._viewshed import _rgba

MAX_SEEDS = 65535
EVERYWHERE, EDGES, SEEDS = 0, 1, 2
MODES = ("everywhere", "edges", "seeds")
DEFAULTS = {"shallow_rgba": (96, 176, 224, 128), "deep_rgba": (16, 64, 160, 224), "depth_full": 0.1}


def seed_list(seeds, what):
    """a seed list of set_flood / set_spill -> (N, 2) float32 C-contiguous, 1 <= N <= MAX_SEEDS, finite.  what: the caller's "seeds
    must be ..." for a value that is no array of numbers."""
    try:
        xz = np.asarray(seeds)
    except Exception:
        raise TypeError(f"{what}, got {type(seeds).__name__}") from None
    if xz.dtype == object or xz.dtype.kind not in "fiu":
        raise TypeError(f"{what}, got dtype {xz.dtype}")
    if xz.ndim != 2 or xz.shape[1] != 2:
        raise ValueError(f"seeds must be (N, 2) numbers, got shape {xz.shape}")
    if not 1 <= xz.shape[0] <= MAX_SEEDS:
        raise ValueError(f"seeds must hold 1 to {MAX_SEEDS} rows, got {xz.shape[0]}")
    xz = np.ascontiguousarray(xz, np.float32)
    if not np.isfinite(xz).all():
        raise ValueError("seeds must be finite")
    return xz


def flood_args(level, seeds=None, enabled=True, shallow_rgba=(96, 176, 224, 128), deep_rgba=(16, 64, 160, 224), depth_full=0.1):
    """-> (enable 0 / 1, level, mode, seeds (N, 2) float32 C-contiguous or None, shallow (r, g, b, a), deep (r, g, b, a), depth_full) as
    the C call takes them.  seeds: None -- everywhere; "edges"; or (N, 2) numbers (x, z)."""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    level = _number("level", level)
    depth_full = _number("depth_full", depth_full)
    if not depth_full > 0.0:
        raise ValueError(f"depth_full must be > 0, got {depth_full}")
    xz = None
    if seeds is None:
        mode = EVERYWHERE
    elif isinstance(seeds, str):
        if seeds != "edges":
            raise ValueError(f'seeds must be None, "edges" or (N, 2) numbers, got {seeds!r}')
        mode = EDGES
    else:
        mode = SEEDS
        xz = seed_list(seeds, 'seeds must be None, "edges" or (N, 2) numbers')
    return (1 if enabled else 0, level, mode, xz, _rgba("shallow_rgba", shallow_rgba), _rgba("deep_rgba", deep_rgba), depth_full)


def flood_info(enabled, has_flood, mode, count, vertices, level, depth_full, shallow_rgba, deep_rgba, flooded_vertices, wettable_vertices, passes,
               scans, group):
    """the C calls' outputs -> the dict flood_info() returns; level and mode are None before a flood is set, vertices is the (N, 2)
    uint32 array of the seeds' vertices (i, j), None without seeds (or before uniforms are set)"""
    return {"enabled": bool(enabled), "level": float(level) if has_flood else None, "mode": MODES[int(mode)] if has_flood else None,
            "seeds": int(count), "vertices": None if vertices is None else np.asarray(vertices, np.uint32).reshape(-1, 2),
            "shallow_rgba": tuple(int(v) for v in shallow_rgba), "deep_rgba": tuple(int(v) for v in deep_rgba), "depth_full": float(depth_full),
            "flooded_vertices": int(flooded_vertices), "wettable_vertices": int(wettable_vertices), "passes": int(passes), "scans": int(scans),
            "group": int(group)}
