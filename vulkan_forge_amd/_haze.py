"""Argument rules of the haze methods (Scene / TerrainSpike .set_haze / .haze_info).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, atmospheric haze); they need no device.
"""
from __future__ import annotations

from ._shadows import _number
from ._viewshed import _rgba

DEFAULTS = {"rgba": (200, 215, 235, 255), "start": 0.0, "falloff": None, "base": 0.0, "max_opacity": 1.0, "background": False}


def haze_args(density, rgba=(200, 215, 235, 255), start=0.0, falloff=None, base=0.0, max_opacity=1.0, background=False, enabled=True):
    """-> (enable 0 / 1, density, (r, g, b, a), start, falloff (0.0: uniform haze), base, max_opacity, background 0 / 1) as the C call
    takes them"""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    if not isinstance(background, (bool, int)):
        raise TypeError(f"background must be a bool, got {type(background).__name__}")
    density, start, base, max_opacity = _number("density", density), _number("start", start), _number("base", base), _number("max_opacity", max_opacity)
    if density < 0.0:
        raise ValueError(f"density must be >= 0, got {density}")
    if start < 0.0:
        raise ValueError(f"start must be >= 0, got {start}")
    if falloff is None:
        falloff = 0.0
    else:
        falloff = _number("falloff", falloff)
        if not falloff > 0.0:
            raise ValueError(f"falloff must be None (uniform haze) or > 0, got {falloff}")
    if not 0.0 <= max_opacity <= 1.0:
        raise ValueError(f"max_opacity must lie in [0, 1], got {max_opacity}")
    return (1 if enabled else 0, density, _rgba("rgba", rgba), start, falloff, base, max_opacity, 1 if background else 0)


def haze_info(enabled, background, density, start, falloff, base, max_opacity, rgba, has_eye, eye_y):
    """the C call's outputs -> the dict haze_info() returns; falloff is None for uniform haze, eye_y None before uniforms are set"""
    return {"enabled": bool(enabled), "density": float(density), "rgba": tuple(int(v) for v in rgba), "start": float(start),
            "falloff": float(falloff) if falloff > 0.0 else None, "base": float(base), "max_opacity": float(max_opacity),
            "background": bool(background), "eye_y": float(eye_y) if has_eye else None}
