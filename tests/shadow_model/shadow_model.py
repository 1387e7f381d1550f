"""ctypes loader of the cast-shadow CPU model (shadow_model.c).

    import shadow_model as shm
    lit = shm.field_heights(h, sun, spacing=1.0, exag=1.0, strength=0.7, softness=0.02, bias=0.002)   # h: (n, n) vertex heights
    lit = shm.field(uniforms, height, grid, strength=..., softness=..., bias=...)                     # the renderer's own surface
    frame, shadowed = shm.frame(rgba, vis, uniforms, height, grid, lut_rgba8, lit, shade_mode=0)

`rgba` is the unshadowed frame (H, W, 4) and `vis` its visibility (H, W) uint32 (oracle.render_terrain); `lut_rgba8` the handle's
256 sRGB texels; `shadowed` marks the pixels whose interpolated lit is below 1 (the ones the shade pass writes again).
"""
from __future__ import annotations

import numpy as np

import model_support as ms

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

SIGNATURES = {
    "shm_field_heights": "i32(f32*, f32*, u32, f32*, f32, f32, f32, f32, f32)",
    "shm_heights": "i32(f32*, f32*, f32*, u32, u32, u32)",
    "shm_frame": "i32(u8*, u8*, u32*, u32, u32, f32*, f32*, u32, u32, u32, u8*, i32, f32*)",
}


def lib():
    return ms.load("shadow_model", SIGNATURES)


def field_heights(h, sun, spacing=1.0, exag=1.0, strength=0.7, softness=0.02, bias=0.002):
    """h (n, n) float32 vertex heights (row = z index, column = x index), sun (3,) -> lit (n, n) float32"""
    h = np.ascontiguousarray(h, np.float32)
    assert h.ndim == 2 and h.shape[0] == h.shape[1]
    sun = np.ascontiguousarray(sun, np.float32).reshape(3)
    lit = np.empty_like(h)
    assert lib().shm_field_heights(lit, h, h.shape[0], sun, spacing, exag, strength, softness, bias) == 0
    return lit


def heights(uniforms, height, grid):
    """the displaced heights the renderer draws, (n, n) float32"""
    n = max(int(grid), 2)
    h = np.empty((n, n), np.float32)
    assert lib().shm_heights(h, ms.u44(uniforms), *ms.texture(height), grid) == 0
    return h


def field(uniforms, height, grid, strength=0.7, softness=0.02, bias=0.002):
    """the field of the renderer's surface for the uniforms' sun, spacing (u[36], at least 1e-8) and exaggeration (u[38])"""
    u = ms.u44(uniforms)
    return field_heights(heights(u, height, grid), u[32:35], float(max(u[36], np.float32(1e-8))), float(u[38]), strength, softness, bias)


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, lit, shade_mode=0):
    """-> (the shadowed frame (H, W, 4) uint8, shadowed (H, W) bool)"""
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    mask = np.empty(vis.shape, np.uint8)
    assert lib().shm_frame(out, mask, vis, *scene, grid, ms.lut(lut_rgba8), int(shade_mode), ms.field(lit)) == 0
    return out, mask.astype(bool)
