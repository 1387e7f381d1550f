"""Argument rules of the viewshed methods (Scene / TerrainSpike .set_viewshed / .viewshed_info).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, viewshed analysis); they need no device.
"""
from __future__ import annotations

from ._shadows import _number

DEFAULTS = {"eye_height": 0.05, "target_height": 0.0, "radius": None, "visible_rgba": (64, 255, 96, 96), "hidden_rgba": (0, 0, 0, 0),
            "softness": 0.02, "bias": 0.002}


def _rgba(name, v):
    try:
        v = tuple(v)
    except TypeError:
        raise TypeError(f"{name} must be 4 ints in 0..255, got {type(v).__name__}") from None
    if len(v) != 4:
        raise ValueError(f"{name} must be 4 ints in 0..255, got {len(v)} values")
    out = []
    for c in v:
        if isinstance(c, bool) or not hasattr(c, "__index__"):
            raise TypeError(f"{name} must be 4 ints in 0..255, got a {type(c).__name__}")
        c = int(c)
        if not 0 <= c <= 255:
            raise ValueError(f"{name} must be 4 ints in 0..255, got {c}")
        out.append(c)
    return tuple(out)


def viewshed_args(observer, enabled=True, eye_height=0.05, target_height=0.0, radius=None, visible_rgba=(64, 255, 96, 96),
                  hidden_rgba=(0, 0, 0, 0), softness=0.02, bias=0.002):
    """-> (enable 0 / 1, x, z, eye_height, target_height, radius (0.0: none), visible (r, g, b, a), hidden (r, g, b, a), softness,
    bias) as the C call takes them"""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    try:
        obs = tuple(observer)
    except TypeError:
        raise TypeError(f"observer must be (x, z), got {type(observer).__name__}") from None
    if len(obs) != 2:
        raise ValueError(f"observer must be (x, z), got {len(obs)} values")
    x, z = _number("observer x", obs[0]), _number("observer z", obs[1])
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
    return (1 if enabled else 0, x, z, eye_height, target_height, radius, _rgba("visible_rgba", visible_rgba), _rgba("hidden_rgba", hidden_rgba),
            softness, bias)


def viewshed_info(enabled, has_observer, vertex, observer_xyz, eye_y, eye_height, target_height, radius, softness, bias, visible_rgba, hidden_rgba):
    """the C call's outputs -> the dict viewshed_info() returns; vertex, observer_xyz and eye_y are None before an observer is set"""
    return {"enabled": bool(enabled),
            "vertex": tuple(int(v) for v in vertex) if has_observer else None,
            "observer_xyz": tuple(float(v) for v in observer_xyz) if has_observer else None,
            "eye_y": float(eye_y) if has_observer else None,
            "eye_height": float(eye_height), "target_height": float(target_height), "radius": float(radius) if radius > 0.0 else None,
            "visible_rgba": tuple(int(v) for v in visible_rgba), "hidden_rgba": tuple(int(v) for v in hidden_rgba),
            "softness": float(softness), "bias": float(bias)}
