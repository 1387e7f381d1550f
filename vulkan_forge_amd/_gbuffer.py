"""Argument rules of the geometry-buffer methods (Scene / TerrainSpike .render_gbuffer / .render_depth / .pick).

The extension calls these before it hands the arrays to the C-ABI (include/vf_hip.h, geometry buffers); they need numpy only, no
device.
"""
from __future__ import annotations

import numpy as np

# plane name -> (dtype, trailing shape), in the order of the C calls' arguments
PLANES = {"depth": (np.float32, ()), "position": (np.float32, (3,)), "normal": (np.float32, (3,)), "primitive": (np.uint32, ())}


def plane_args(planes):
    """-> the requested plane names as a tuple, in the caller's order"""
    if isinstance(planes, str):
        raise TypeError(f"planes must be a sequence of plane names, got the string {planes!r}")
    try:
        names = tuple(planes)
    except TypeError:
        raise TypeError(f"planes must be a sequence of plane names, got {type(planes).__name__}") from None
    if not names:
        raise ValueError(f"planes must name at least one of {list(PLANES)}")
    for k in names:
        if not isinstance(k, str):
            raise TypeError(f"plane names must be strings, got {k!r}")
        if k not in PLANES:
            raise ValueError(f"unknown plane {k!r}: planes are {list(PLANES)}")
    if len(set(names)) != len(names):
        raise ValueError(f"planes names {[k for k in PLANES if names.count(k) > 1][0]!r} more than once")
    return names


def pixel_args(pixels, width, height):
    """-> pixels as a C-contiguous (N, 2) int32 array of (x, y), every one inside the width x height frame"""
    a = pixels if isinstance(pixels, np.ndarray) else np.asarray(pixels)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        if a.size == 0 and not isinstance(pixels, np.ndarray):
            a = a.astype(np.int32)                            # (an empty list has no dtype of its own)
        else:
            raise TypeError(f"pixels must be an integer array, got dtype {a.dtype}")
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"pixels must have shape (N, 2) of (x, y), got {a.shape}")
    if len(a):
        outside = (a[:, 0] < 0) | (a[:, 0] >= width) | (a[:, 1] < 0) | (a[:, 1] >= height)
        if outside.any():
            k = int(np.argmax(outside))
            raise ValueError(f"pixel {k} ({int(a[k, 0])}, {int(a[k, 1])}) lies outside the {width} x {height} frame")
    return np.ascontiguousarray(a, dtype=np.int32)


def pick_result(words):
    """(N, 8) uint32 records {depth, x, y, z, nx, ny, nz, id} -> dict of depth (N,), position (N, 3), normal (N, 3), primitive (N,)"""
    f = words.view(np.float32)
    return {"depth": f[:, 0].copy(), "position": f[:, 1:4].copy(), "normal": f[:, 4:7].copy(), "primitive": words[:, 7].copy()}
