"""Argument rules of supersampled terrain frames (Scene / TerrainSpike(..., supersample=f)).

The extension calls these before it hands the sizes to the C-ABI (include/vf_hip.h, supersampled terrain frames); they need no
device.
"""
from __future__ import annotations

import operator

SUPERSAMPLE_MAX = 4          # VF_SUPERSAMPLE_MAX
FRAME_LIMIT = 16384          # the frame limit of vf_terrain_create, which the sample size has to meet


def supersample_args(width, height, supersample):
    """-> the factor f as an int in 1..SUPERSAMPLE_MAX with f * width and f * height inside the frame limit"""
    if isinstance(supersample, bool):
        raise TypeError("supersample must be an integer, got a bool")
    try:
        f = operator.index(supersample)
    except TypeError:
        raise TypeError(f"supersample must be an integer, got {type(supersample).__name__}") from None
    if not 1 <= f <= SUPERSAMPLE_MAX:
        raise ValueError(f"supersample must be in 1..{SUPERSAMPLE_MAX}, got {f}")
    w, h = int(width), int(height)
    if f > 1 and (f * w > FRAME_LIMIT or f * h > FRAME_LIMIT):
        raise ValueError(f"supersample={f} on a {w} x {h} frame needs {f * w} x {f * h} samples: more than the {FRAME_LIMIT} x {FRAME_LIMIT} limit")
    return f


def sample_size(width, height, supersample):
    """(f * width, f * height): the size the terrain is drawn at"""
    f = supersample_args(width, height, supersample)
    return f * int(width), f * int(height)


def representative(x, y, supersample):
    """the sample pick() answers for at output pixel (x, y): (f x + f // 2, f y + f // 2)"""
    f = int(supersample)
    return f * int(x) + f // 2, f * int(y) + f // 2
