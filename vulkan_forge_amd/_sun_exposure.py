"""Argument rules of the sun exposure methods (Scene / TerrainSpike .set_sun_exposure / .sun_exposure_info).

The extension calls these before it hands the values to the C-ABI (include/vf_hip.h, sun exposure); they need no device.
"""
from __future__ import annotations

import numpy as np

from ._shadows import _number
from ._viewshed import _rgba

MAX_SUNS = 65535
DEFAULTS = {"weights": None, "incidence": False, "softness": 0.02, "bias": 0.002, "high_rgba": (255, 208, 64, 160), "low_rgba": (0, 0, 0, 0)}


def sun_exposure_args(suns, weights=None, incidence=False, enabled=True, softness=0.02, bias=0.002, high_rgba=(255, 208, 64, 160),
                      low_rgba=(0, 0, 0, 0)):
    """-> (enable 0 / 1, suns float32 C-contiguous -- (N, 2) angles (elevation_deg, azimuth_deg), which the caller turns into vectors as
    set_sun does, or (N, 3) vectors --, weights (N,) float32, incidence 0 / 1, softness, bias, high (r, g, b, a), low (r, g, b, a))"""
    if not isinstance(enabled, (bool, int)):
        raise TypeError(f"enabled must be a bool, got {type(enabled).__name__}")
    if not isinstance(incidence, (bool, int)):
        raise TypeError(f"incidence must be a bool, got {type(incidence).__name__}")
    try:
        s = np.asarray(suns)
    except Exception:
        raise TypeError(f"suns must be (N, 2) angles or (N, 3) vectors, got {type(suns).__name__}") from None
    if s.dtype == object or s.dtype.kind not in "fiu":
        raise TypeError(f"suns must be (N, 2) angles or (N, 3) vectors, got dtype {s.dtype}")
    if s.ndim != 2 or s.shape[1] not in (2, 3):
        raise ValueError(f"suns must be (N, 2) angles or (N, 3) vectors, got shape {s.shape}")
    if not 1 <= s.shape[0] <= MAX_SUNS:
        raise ValueError(f"suns must hold 1 to {MAX_SUNS} rows, got {s.shape[0]}")
    with np.errstate(over="ignore"):
        s = np.ascontiguousarray(s, np.float32)
    if not np.isfinite(s).all():
        raise ValueError("suns must be finite")
    if weights is None:
        w = np.ones(s.shape[0], np.float32)
    else:
        try:
            w = np.asarray(weights)
        except Exception:
            raise TypeError(f"weights must be (N,) numbers, got {type(weights).__name__}") from None
        if w.dtype == object or w.dtype.kind not in "fiu":
            raise TypeError(f"weights must be (N,) numbers, got dtype {w.dtype}")
        if w.shape != (s.shape[0],):
            raise ValueError(f"weights must have shape ({s.shape[0]},), one per sun, got {w.shape}")
        w = np.ascontiguousarray(w, np.float32)
        if not (np.isfinite(w).all() and (w >= 0.0).all() and (w <= 1.0).all()):
            raise ValueError("weights must be finite and lie in [0, 1]")
    softness, bias = _number("softness", softness), _number("bias", bias)
    if not softness > 0.0:
        raise ValueError(f"softness must be > 0, got {softness}")
    if bias < 0.0:
        raise ValueError(f"bias must be >= 0, got {bias}")
    return (1 if enabled else 0, s, w, 1 if incidence else 0, softness, bias, _rgba("high_rgba", high_rgba), _rgba("low_rgba", low_rgba))


def sun_exposure_info(enabled, count, counted, weight_total, incidence, batch, softness, bias, high_rgba, low_rgba):
    """the C call's outputs -> the dict sun_exposure_info() returns"""
    return {"enabled": bool(enabled), "suns": int(count), "counted": int(counted), "weight_total": float(weight_total),
            "incidence": bool(incidence), "batch": int(batch), "softness": float(softness), "bias": float(bias),
            "high_rgba": tuple(int(v) for v in high_rgba), "low_rgba": tuple(int(v) for v in low_rgba)}
