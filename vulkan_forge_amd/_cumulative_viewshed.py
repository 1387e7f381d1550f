"""Argument rules of the cumulative viewshed methods (Scene / TerrainSpike .set_cumulative_viewshed / .cumulative_viewshed_info;
DESIGN.md 4m).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, cumulative viewsheds); they need no device.
"""
from __future__ import annotations

import numpy as np

from ._shadows import _number
from ._viewshed import _rgba

MAX_OBSERVERS = 65535
DEFAULTS = {"eye_height": 0.05, "target_height": 0.0, "radius": None, "high_rgba": (64, 255, 96, 160), "low_rgba": (0, 0, 0, 0),
            "softness": 0.02, "bias": 0.002}


def cumulative_viewshed_args(observers, enabled=True, eye_height=0.05, target_height=0.0, radius=None, high_rgba=(64, 255, 96, 160),
                             low_rgba=(0, 0, 0, 0), softness=0.02, bias=0.002):
    """-> (enable 0 / 1, observers (N, 2) float32 C-contiguous, eye_height, target_height, radius (0.0: none), high (r, g, b, a),
    low (r, g, b, a), softness, bias) as the C call takes them"""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    try:
        obs = np.asarray(observers)
    except Exception:
        raise TypeError(f"observers must be (N, 2) numbers, got {type(observers).__name__}") from None
    if obs.dtype == object or obs.dtype.kind not in "fiu":
        raise TypeError(f"observers must be (N, 2) numbers, got dtype {obs.dtype}")
    if obs.ndim != 2 or obs.shape[1] != 2:
        raise ValueError(f"observers must be (N, 2) numbers, got shape {obs.shape}")
    if not 1 <= obs.shape[0] <= MAX_OBSERVERS:
        raise ValueError(f"observers must hold 1 to {MAX_OBSERVERS} rows, got {obs.shape[0]}")
    obs = np.ascontiguousarray(obs, np.float32)
    if not np.isfinite(obs).all():
        raise ValueError("observers must be finite")
    eye_height, target_height = _number("eye_height", eye_height), _number("target_height", target_height)
    softness, bias = _number("softness", softness), _number("bias", bias)
    if eye_height < 0.0:
        raise ValueError(f"eye_height must be >= 0, got {eye_height}")
    if target_height < 0.0:
        raise ValueError(f"target_height must be >= 0, got {target_height}")
    if radius is None:
        radius = 0.0
    else:
        radius = _number("radius", radius)
        if not radius > 0.0:
            raise ValueError(f"radius must be None or > 0, got {radius}")
    if not softness > 0.0:
        raise ValueError(f"softness must be > 0, got {softness}")
    if bias < 0.0:
        raise ValueError(f"bias must be >= 0, got {bias}")
    return (1 if enabled else 0, obs, eye_height, target_height, radius, _rgba("high_rgba", high_rgba), _rgba("low_rgba", low_rgba), softness, bias)


def cumulative_viewshed_info(enabled, count, batch, vertices, eye_height, target_height, radius, softness, bias, high_rgba, low_rgba):
    """the C calls' outputs -> the dict cumulative_viewshed_info() returns; vertices is the (N, 2) uint32 array of the observers'
    vertices (i, j), None before observers (and uniforms) are set"""
    return {"enabled": bool(enabled), "observers": int(count), "batch": int(batch),
            "vertices": None if vertices is None else np.asarray(vertices, np.uint32).reshape(-1, 2),
            "eye_height": float(eye_height), "target_height": float(target_height), "radius": float(radius) if radius > 0.0 else None,
            "high_rgba": tuple(int(v) for v in high_rgba), "low_rgba": tuple(int(v) for v in low_rgba),
            "softness": float(softness), "bias": float(bias)}
