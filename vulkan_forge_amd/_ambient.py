"""Argument rules of the ambient-occlusion methods (Scene / TerrainSpike .set_ambient_occlusion).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, ambient occlusion); they need no device.
"""
from __future__ import annotations

import math

import numpy as np

from ._shadows import _number

DEFAULTS = {"strength": 0.6, "reach": 64.0, "directions": 16}
MAX_DIRECTIONS = 64


def directions(D):
    """The default set: D horizontal directions (ux, uz) at azimuth 360 t / D degrees, (D, 2) float32.  Computed in float64 and
    rounded; multiples of 90 degrees are the exact axes and odd multiples of 45 degrees (+-1, +-1): the lines of such a direction
     depend on the ratio of the components alone, and these ratios are exact."""
    if isinstance(D, bool) or not isinstance(D, (int, np.integer)):
        raise TypeError(f"directions must be an int or a (D, 2) array, got {type(D).__name__}")
    D = int(D)
    if not 1 <= D <= MAX_DIRECTIONS:
        raise ValueError(f"directions must lie in [1, {MAX_DIRECTIONS}], got {D}")
    out = np.empty((D, 2), np.float32)
    for t in range(D):
        if (8 * t) % D == 0:                              # a whole number of octants
            o = 8 * t // D
            out[t] = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))[o]
        else:
            az = 2.0 * math.pi * t / D
            out[t] = (math.cos(az), math.sin(az))
    return out


def ambient_args(enabled, strength, reach, dirs):
    """-> (enable 0 / 1, strength, reach, D, (D, 2) float32 array) as the C call takes them"""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    strength, reach = _number("strength", strength), _number("reach", reach)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"strength must lie in [0, 1], got {strength}")
    if not 1.0 <= reach <= 1024.0:
        raise ValueError(f"reach must lie in [1, 1024], got {reach}")
    if isinstance(dirs, (int, np.integer)) and not isinstance(dirs, bool):
        d = directions(dirs)
    else:
        try:
            d = np.ascontiguousarray(dirs, np.float32)
        except (TypeError, ValueError):
            raise TypeError(f"directions must be an int or a (D, 2) array, got {type(dirs).__name__}") from None
        if d.ndim != 2 or d.shape[1] != 2:
            raise ValueError(f"directions must be an int or a (D, 2) array, got shape {d.shape}")
        if not 1 <= len(d) <= MAX_DIRECTIONS:
            raise ValueError(f"directions must lie in [1, {MAX_DIRECTIONS}], got {len(d)}")
        if not np.isfinite(d).all():
            raise ValueError("directions must be finite")
        if (~d.any(axis=1)).any():
            raise ValueError("a direction needs a horizontal part: (0, 0) is none")
    return (1 if enabled else 0, strength, reach, len(d), d)
