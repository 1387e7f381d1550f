"""ctypes loader of the ambient-occlusion CPU model (ambient_model.c).

    import ambient_model as abm
    sky = abm.field_heights(h, dirs, spacing=1.0, exag=1.0, reach=64.0)          # h: (n, n) vertex heights, dirs: (D, 2) float32
    sky = abm.field(uniforms, height, grid, dirs, reach=...)                     # the renderer's own surface
    frame, rewritten = abm.frame(rgba, vis, uniforms, height, grid, lut_rgba8, sky, strength, lit=None, shade_mode=0)

`rgba` is the plain frame (H, W, 4) and `vis` its visibility (H, W) uint32 (oracle.render_terrain); `lit` the shadow field when cast
shadows are on as well; `rewritten` marks the pixels whose interpolated lit or amb is below 1 (the ones the shade pass writes again).
"""
from __future__ import annotations

import numpy as np

import model_support as ms
import overlay_scenes
import shadow_model as shm

# The GPU field tests: (grid, exaggeration, reach, D) on overlay_scenes.heights(4, (97, 131)) -- a grid that is no multiple of 8 or 64,
# a reach that crosses one tile boundary, one that crosses two, many chunks plus one, and a single direction.
FIELD_CASES = [(203, 0.6, 16.0, 16), (130, 0.6, 70.0, 16), (520, 0.6, 130.0, 16), (1025, 0.6, 20.0, 16), (203, 0.6, 16.0, 1)]
# The same at the limits the C ABI accepts (tests/test_gpu_limits.py): reach 1024 cells on a grid that does not clip it, along one x-major
# and one z-major axis direction and along the diagonal (a list of directions in place of a count), and 64 directions.  At reach 1024
# a vertex's scan looks back over 1024 / 64 = 16 earlier tiles, which is what the kernel's table is sized for.  On limit_heights():
# over white noise, and over the analytic surface's hill along z, every horizon is a few cells away and the far tiles of the scan
# decide nothing; in a bowl the rim is the horizon of the vertices that look across it, and the field of reach 1024 differs from
# the one of reach 512 at 29-51 % of the vertices (test_ambient_model.py asserts more than 10 % on the same surface at a quarter of
# the grid and of the reach, which costs a sixty-fourth).
LIMIT_FIELD_CASES = [(1100, 0.6, 1024.0, ((1, 0),)), (1100, 0.6, 1024.0, ((0, -1),)), (1100, 0.6, 1024.0, ((1, 1),)), (203, 0.6, 16.0, 64)]


def limit_heights():
    """the texture of LIMIT_FIELD_CASES: a bowl of depth 2 over the texture's square, and overlay_scenes' noise at a fiftieth of its height"""
    v, u = np.meshgrid(np.linspace(-1.0, 1.0, 97), np.linspace(-1.0, 1.0, 131), indexing="ij")
    return (overlay_scenes.heights(4, (97, 131)) * np.float32(0.02) + (u * u + v * v)).astype(np.float32)


def case_directions(D):
    """the (D, 2) float32 directions of a field case: the library's default set of D, or the case's own list"""
    if isinstance(D, int):
        from vulkan_forge_amd._ambient import directions
        return directions(D)
    return np.array(D, np.float32).reshape(-1, 2)


# an exact diagonal, both axes, a nearly-axis direction in each major axis, general ones in other quadrants, none normalised
IRREGULAR = np.array([(1, 1), (1, 0), (0, -1), (1, 1e-3), (-2e-3, 1), (-0.9, 0.31), (0.31, -0.9), (-3, -3), (0, 2)], np.float32)
# The GPU frame tests' scene: overlay_scenes' white noise at a hundredth of its height, so that the analytic surface under it shows.
# Every slope of a rough or smooth surface is seen from somewhere, so an all-round direction set leaves no vertex with an open sky and
# every pixel would be written again; these three directions look one way, down the analytic surface over most of the grid, and
# between 10 % and 90 % of the covered pixels of every test camera are written again while more than 10 % of the vertices have a
# sky view in (0.1, 0.9) (test_ambient_model.py asserts both).
SCENE_PARAMS = dict(strength=0.8, reach=2.0)
SCENE_SUN_DEG = (8.0, 30.0)                                # elevation, azimuth: low enough for the analytic surface to cast shadows
SCENE_SHADOWS = dict(strength=0.7, softness=0.02, bias=0.001)


def scene_directions():
    return np.array([(-1, 0), (-0.9, 0.31), (-0.9, -0.31)], np.float32)


def scene_heights(seed=7):
    return (overlay_scenes.heights(seed) * np.float32(0.01)).astype(np.float32)


SIGNATURES = {
    "abm_field_heights": "i32(f32*, f32*, u32, f32*, u32, f32, f32, f32)",
    "abm_frame": "i32(u8*, u8*, u32*, u32, u32, f32*, f32*, u32, u32, u32, u8*, i32, f32*?, f32*, f32)",
}


def lib():
    return ms.load("ambient_model", SIGNATURES)


def field_heights(h, dirs, spacing=1.0, exag=1.0, reach=64.0):
    """h (n, n) float32 vertex heights (row = z index, column = x index), dirs (D, 2) float32 -> sky (n, n) float32"""
    h = np.ascontiguousarray(h, np.float32)
    assert h.ndim == 2 and h.shape[0] == h.shape[1]
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 2)
    sky = np.empty_like(h)
    if lib().abm_field_heights(sky, h, h.shape[0], dirs, len(dirs), spacing, exag, reach) != 0:
        raise ValueError("a direction without a horizontal part, or a non-finite one")
    return sky


def field(uniforms, height, grid, dirs, reach=64.0):
    """the field of the renderer's surface for the uniforms' spacing (u[36], at least 1e-8) and exaggeration (u[38])"""
    u = ms.u44(uniforms)
    return field_heights(shm.heights(u, height, grid), dirs, float(max(u[36], np.float32(1e-8))), float(u[38]), reach)


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, sky, strength, lit=None, shade_mode=0):
    """-> (the frame with ambient occlusion (H, W, 4) uint8, rewritten (H, W) bool)"""
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    mask = np.empty(vis.shape, np.uint8)
    assert lib().abm_frame(out, mask, vis, *scene, grid, ms.lut(lut_rgba8), int(shade_mode), ms.field(lit), ms.field(sky), strength) == 0
    return out, mask.astype(bool)
