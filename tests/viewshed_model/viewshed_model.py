"""ctypes loader of the viewshed CPU model (viewshed_model.c).

    seen = vsm.field_heights(h, (io, jo), exag=1.0, eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002)   # h: (n, n) vertex heights
    seen, (io, jo) = vsm.field(uniforms, height, grid, observer=(x, z), eye_height=..., ...)                        # the renderer's own surface
    frame, s = vsm.frame(rgba, vis, uniforms, height, grid, seen, (io, jo), radius=None, visible_rgba=..., hidden_rgba=...)

`rgba` is the untinted frame (H, W, 4) and `vis` its visibility (H, W) uint32; `s` (H, W) float32 is each pixel's seen value, -1 where
the tint pass does not treat the pixel (background, or outside the radius).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "shadow_model"))
import shadow_model as shm  # noqa: E402
om = shm.om

DEFAULTS = dict(eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002)
DEFAULT_VISIBLE, DEFAULT_HIDDEN = (64, 255, 96, 96), (0, 0, 0, 0)
# The GPU tests' scene (overlay_scenes.heights() on GRID vertices) is white noise on four-vertex plateaus of +-0.3: from an eye near
# the ground nearly everything is hidden.  From this observer, raised above the noise, between 10 % and 90 % of the covered pixels of
# every test camera are hidden (s < 0.5; test_viewshed_model.py asserts it).
SCENE_OBSERVER = (0.4, 0.3)
SCENE_PARAMS = dict(eye_height=1.0, target_height=0.0, softness=0.1, bias=0.01)

_lib = None


def lib():
    global _lib
    if _lib is None:
        T = os.path.dirname(HERE)
        L = om.build_model("libvsmodel.so", os.path.join(HERE, "viewshed_model.c"),
                           [os.path.join(T, "shadow_model", "shadow_model.c"), os.path.join(T, "gbuffer_model", "gbuffer_model.c"),
                            os.path.join(T, "occlusion_model", "occlusion_model.c"), os.path.join(T, "polygon_model", "polygon_model.c"),
                            os.path.join(T, "overlay_model", "overlay_model.c")])
        vp, u32, i32, f, i = C.c_void_p, C.c_uint32, C.c_int32, C.c_float, C.c_int
        L.vsm_observer_index.argtypes = [f, f, u32]
        L.vsm_observer_index.restype = u32
        L.vsm_minor.argtypes = [u32, i32, u32]
        L.vsm_minor.restype = i32
        L.vsm_owner.argtypes = [u32, u32, i32]
        L.vsm_owner.restype = i32
        L.vsm_field_heights.argtypes = [vp, vp, vp, u32, u32, u32, f, f, f, f, f]
        L.vsm_field_heights.restype = i
        L.vsm_frame.argtypes = [vp, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, u32, u32, f, u32, u32]
        L.vsm_frame.restype = i
        _lib = L
    return _lib


def pack(rgba):
    r, g, b, a = (int(v) for v in rgba)
    return r | g << 8 | b << 16 | a << 24


def observer_vertex(observer, spacing, n):
    """(x, z) in the overlays' world frame -> the observer's vertex (io, jo)"""
    return (int(lib().vsm_observer_index(float(observer[0]), float(spacing), n)), int(lib().vsm_observer_index(float(observer[1]), float(spacing), n)))


def field_heights(h, vertex, exag=1.0, eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002, writers=False):
    """h (n, n) float32 vertex heights (row = z index, column = x index), vertex (io, jo) -> seen (n, n) float32
    (and, with writers, how many (line, step) pairs own each vertex)"""
    h = np.ascontiguousarray(h, np.float32)
    assert h.ndim == 2 and h.shape[0] == h.shape[1]
    seen = np.empty_like(h)
    w = np.empty(h.shape, np.uint32) if writers else None
    assert lib().vsm_field_heights(seen.ctypes.data, w.ctypes.data if writers else None, h.ctypes.data, h.shape[0], int(vertex[0]), int(vertex[1]),
                                   exag, eye_height, target_height, softness, bias) == 0
    return (seen, w) if writers else seen


def field(uniforms, height, grid, observer, eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002):
    """the field of the renderer's surface for the uniforms' spacing (u[36], at least 1e-8) and exaggeration (u[38]) -> (seen, (io, jo))"""
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    n = max(int(grid), 2)
    v = observer_vertex(observer, max(u[36], np.float32(1e-8)), n)
    return field_heights(shm.heights(u, height, grid), v, float(u[38]), eye_height, target_height, softness, bias), v


def frame(rgba, vis, uniforms, height, grid, seen, vertex, radius=None, visible_rgba=DEFAULT_VISIBLE, hidden_rgba=DEFAULT_HIDDEN):
    """-> (the tinted frame (H, W, 4) uint8, s (H, W) float32)"""
    vis = np.ascontiguousarray(vis, np.uint32)
    H, W = vis.shape
    out = np.ascontiguousarray(rgba, np.uint8).reshape(H, W, 4).copy()
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    seen = np.ascontiguousarray(seen, np.float32)
    s = np.empty((H, W), np.float32)
    assert lib().vsm_frame(out.ctypes.data, s.ctypes.data, vis.ctypes.data, W, H, u.ctypes.data, tex.ctypes.data, tex.shape[1], tex.shape[0], grid,
                           seen.ctypes.data, int(vertex[0]), int(vertex[1]), 0.0 if radius is None else float(radius), pack(visible_rgba),
                           pack(hidden_rgba)) == 0
    return out, s
