"""ctypes loader of the viewshed CPU model (viewshed_model.c).

    seen = vsm.field_heights(h, (io, jo), exag=1.0, eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002)   # h: (n, n) vertex heights
    seen, (io, jo) = vsm.field(uniforms, height, grid, observer=(x, z), eye_height=..., ...)                        # the renderer's own surface
    frame, s = vsm.frame(rgba, vis, uniforms, height, grid, seen, (io, jo), radius=None, visible_rgba=..., hidden_rgba=...)

`rgba` is the untinted frame (H, W, 4) and `vis` its visibility (H, W) uint32; `s` (H, W) float32 is each pixel's seen value, -1 where
the tint pass does not treat the pixel (background, or outside the radius).
"""
from __future__ import annotations

import numpy as np

import model_support as ms
import shadow_model as shm

DEFAULTS = dict(eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002)
DEFAULT_VISIBLE, DEFAULT_HIDDEN = (64, 255, 96, 96), (0, 0, 0, 0)
# The GPU tests' scene (overlay_scenes.heights() on GRID vertices) is white noise on four-vertex plateaus of +-0.3: from an eye near
# the ground nearly everything is hidden.  From this observer, raised above the noise, between 10 % and 90 % of the covered pixels of
# every test camera are hidden (s < 0.5; test_viewshed_model.py asserts it).
SCENE_OBSERVER = (0.4, 0.3)
SCENE_PARAMS = dict(eye_height=1.0, target_height=0.0, softness=0.1, bias=0.01)

SIGNATURES = {
    "vsm_observer_index": "u32(f32, f32, u32)",
    "vsm_minor": "i32(u32, i32, u32)",
    "vsm_owner": "i32(u32, u32, i32)",
    "vsm_field_heights": "i32(f32*, u32*?, f32*, u32, u32, u32, f32, f32, f32, f32, f32)",
    "vsm_frame": "i32(u8*, f32*, u32*, u32, u32, f32*, f32*, u32, u32, u32, f32*, u32, u32, f32, u32, u32)",
}
pack = ms.pack


def lib():
    return ms.load("viewshed_model", SIGNATURES)


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
    assert lib().vsm_field_heights(seen, w, h, h.shape[0], int(vertex[0]), int(vertex[1]), exag, eye_height, target_height, softness, bias) == 0
    return (seen, w) if writers else seen


def field(uniforms, height, grid, observer, eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002):
    """the field of the renderer's surface for the uniforms' spacing (u[36], at least 1e-8) and exaggeration (u[38]) -> (seen, (io, jo))"""
    u = ms.u44(uniforms)
    n = max(int(grid), 2)
    v = observer_vertex(observer, max(u[36], np.float32(1e-8)), n)
    return field_heights(shm.heights(u, height, grid), v, float(u[38]), eye_height, target_height, softness, bias), v


def frame(rgba, vis, uniforms, height, grid, seen, vertex, radius=None, visible_rgba=DEFAULT_VISIBLE, hidden_rgba=DEFAULT_HIDDEN):
    """-> (the tinted frame (H, W, 4) uint8, s (H, W) float32)"""
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    s = np.empty(vis.shape, np.float32)
    assert lib().vsm_frame(out, s, vis, *scene, grid, ms.field(seen), int(vertex[0]), int(vertex[1]), 0.0 if radius is None else float(radius),
                           pack(visible_rgba), pack(hidden_rgba)) == 0
    return out, s
