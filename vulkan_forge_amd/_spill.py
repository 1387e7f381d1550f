"""Argument rules of the spill methods (Scene / TerrainSpike .set_spill / .spill_info).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, spill analysis); they need no device.
"""
from __future__ import annotations

import numpy as np

from ._flood import MAX_SEEDS, seed_list
from ._shadows import _number
from ._viewshed import _rgba

EDGES, SEEDS = 1, 2
MODES = {EDGES: "edges", SEEDS: "seeds"}
DEFAULTS = {"shallow_rgba": (96, 176, 224, 128), "deep_rgba": (16, 64, 160, 224), "depth_full": 0.1}


def spill_args(seeds="edges", enabled=True, shallow_rgba=(96, 176, 224, 128), deep_rgba=(16, 64, 160, 224), depth_full=0.1):
    """-> (enable 0 / 1, mode, seeds (N, 2) float32 C-contiguous or None, shallow (r, g, b, a), deep (r, g, b, a), depth_full) as the C
    call takes them.  seeds: "edges", or (N, 2) numbers (x, z).  There is no `everywhere` mode: its field would be h."""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    depth_full = _number("depth_full", depth_full)
    if not depth_full > 0.0:
        raise ValueError(f"depth_full must be > 0, got {depth_full}")
    xz = None
    if seeds is None:
        raise ValueError('seeds must be "edges" or (N, 2) numbers, got None (with every vertex a source the spill is the height)')
    if isinstance(seeds, str):
        if seeds != "edges":
            raise ValueError(f'seeds must be "edges" or (N, 2) numbers, got {seeds!r}')
        mode = EDGES
    else:
        mode = SEEDS
        xz = seed_list(seeds, 'seeds must be "edges" or (N, 2) numbers')
    return (1 if enabled else 0, mode, xz, _rgba("shallow_rgba", shallow_rgba), _rgba("deep_rgba", deep_rgba), depth_full)


def spill_info(enabled, has_spill, mode, count, vertices, depth_full, shallow_rgba, deep_rgba, reached_vertices, sink_vertices, passes, scans,
               group, tile_runs):
    """the C calls' outputs -> the dict spill_info() returns; mode is None before the spill is set, vertices is the (N, 2) uint32
    array of the seeds' vertices (i, j), None without seeds (or before uniforms are set)"""
    return {"enabled": bool(enabled), "mode": MODES[int(mode)] if has_spill else None,
            "seeds": int(count), "vertices": None if vertices is None else np.asarray(vertices, np.uint32).reshape(-1, 2),
            "shallow_rgba": tuple(int(v) for v in shallow_rgba), "deep_rgba": tuple(int(v) for v in deep_rgba), "depth_full": float(depth_full),
            "reached_vertices": int(reached_vertices), "sink_vertices": int(sink_vertices), "passes": int(passes), "scans": int(scans),
            "group": int(group), "tile_runs": int(tile_runs)}
