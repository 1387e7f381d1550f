"""ctypes loader of the cast-shadow CPU model (shadow_model.c).

    import shadow_model as shm
    lit = shm.field_heights(h, sun, spacing=1.0, exag=1.0, strength=0.7, softness=0.02, bias=0.002)   # h: (n, n) vertex heights
    lit = shm.field(uniforms, height, grid, strength=..., softness=..., bias=...)                     # the renderer's own surface
    frame, shadowed = shm.frame(rgba, vis, uniforms, height, grid, lut_rgba8, lit, shade_mode=0)

`rgba` is the unshadowed frame (H, W, 4) and `vis` its visibility (H, W) uint32 (oracle.render_terrain); `lut_rgba8` the handle's
256 sRGB texels; `shadowed` marks the pixels whose interpolated lit is below 1 (the ones the shade pass writes again).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "gbuffer_model"))
import gbuffer_model as gbm  # noqa: E402
om = gbm.om

DEFAULTS = dict(strength=0.7, softness=0.02, bias=0.002)
# The GPU tests' scene (overlay_scenes.heights() on GRID vertices) is white noise on four-vertex plateaus: slopes of about 100.  Under
# this sun, with this bias, between 10 % and 90 % of the covered pixels of every test camera are shadowed (test_shadow_model.py
# asserts it).
SCENE_SUN_DEG = (80.0, 30.0)                              # elevation, azimuth
SCENE_PARAMS = dict(strength=0.7, softness=0.1, bias=0.3)


def sun_vector(elevation_deg, azimuth_deg):
    """Renderer.set_sun's formula in binary32 (the library's own may differ from it in the last bit of cos / sin)"""
    k = np.float32(3.14159265358979323846) / np.float32(180.0)
    el, az = np.float32(elevation_deg) * k, np.float32(azimuth_deg) * k
    v = np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)], np.float32)
    return v / np.sqrt((v * v).sum(dtype=np.float32))

_lib = None


def lib():
    global _lib
    if _lib is None:
        T = os.path.dirname(HERE)
        L = om.build_model("libshmodel.so", os.path.join(HERE, "shadow_model.c"),
                           [os.path.join(T, "gbuffer_model", "gbuffer_model.c"), os.path.join(T, "occlusion_model", "occlusion_model.c"),
                            os.path.join(T, "polygon_model", "polygon_model.c"), os.path.join(T, "overlay_model", "overlay_model.c")])
        vp, u32, f, i = C.c_void_p, C.c_uint32, C.c_float, C.c_int
        L.shm_field_heights.argtypes = [vp, vp, u32, vp, f, f, f, f, f]
        L.shm_field_heights.restype = i
        L.shm_heights.argtypes = [vp, vp, vp, u32, u32, u32]
        L.shm_heights.restype = i
        L.shm_frame.argtypes = [vp, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, i, vp]
        L.shm_frame.restype = i
        _lib = L
    return _lib


def field_heights(h, sun, spacing=1.0, exag=1.0, strength=0.7, softness=0.02, bias=0.002):
    """h (n, n) float32 vertex heights (row = z index, column = x index), sun (3,) -> lit (n, n) float32"""
    h = np.ascontiguousarray(h, np.float32)
    assert h.ndim == 2 and h.shape[0] == h.shape[1]
    sun = np.ascontiguousarray(sun, np.float32).reshape(3)
    lit = np.empty_like(h)
    assert lib().shm_field_heights(lit.ctypes.data, h.ctypes.data, h.shape[0], sun.ctypes.data, spacing, exag, strength, softness, bias) == 0
    return lit


def heights(uniforms, height, grid):
    """the displaced heights the renderer draws, (n, n) float32"""
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    n = max(int(grid), 2)
    h = np.empty((n, n), np.float32)
    assert lib().shm_heights(h.ctypes.data, u.ctypes.data, tex.ctypes.data, tex.shape[1], tex.shape[0], grid) == 0
    return h


def field(uniforms, height, grid, strength=0.7, softness=0.02, bias=0.002):
    """the field of the renderer's surface for the uniforms' sun, spacing (u[36], at least 1e-8) and exaggeration (u[38])"""
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    return field_heights(heights(u, height, grid), u[32:35], float(max(u[36], np.float32(1e-8))), float(u[38]), strength, softness, bias)


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, lit, shade_mode=0):
    """-> (the shadowed frame (H, W, 4) uint8, shadowed (H, W) bool)"""
    vis = np.ascontiguousarray(vis, np.uint32)
    H, W = vis.shape
    out = np.ascontiguousarray(rgba, np.uint8).reshape(H, W, 4).copy()
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    lut = np.ascontiguousarray(lut_rgba8, np.uint8).reshape(1024)
    lit = np.ascontiguousarray(lit, np.float32)
    mask = np.empty((H, W), np.uint8)
    assert lib().shm_frame(out.ctypes.data, mask.ctypes.data, vis.ctypes.data, W, H, u.ctypes.data, tex.ctypes.data, tex.shape[1], tex.shape[0],
                           grid, lut.ctypes.data, int(shade_mode), lit.ctypes.data) == 0
    return out, mask.astype(bool)
