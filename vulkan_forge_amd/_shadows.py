"""Argument rules of the shadow methods (Scene / TerrainSpike .set_shadows / .set_sun / .set_exposure).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, cast sun shadows); they need no device.
"""
from __future__ import annotations

import math

DEFAULTS = {"strength": 0.7, "softness": 0.02, "bias": 0.002}


def _number(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        try:
            v = float(v)                                  # (numpy scalars)
        except (TypeError, ValueError):
            raise TypeError(f"{name} must be a number, got {type(v).__name__}") from None
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be finite, got {v}")
    return v


def shadow_args(enabled, strength, softness, bias):
    """-> (enable 0 / 1, strength, softness, bias) as the C call takes them"""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    strength, softness, bias = _number("strength", strength), _number("softness", softness), _number("bias", bias)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"strength must lie in [0, 1], got {strength}")
    if not softness > 0.0:
        raise ValueError(f"softness must be > 0, got {softness}")
    if bias < 0.0:
        raise ValueError(f"bias must be >= 0, got {bias}")
    return (1 if enabled else 0, strength, softness, bias)
