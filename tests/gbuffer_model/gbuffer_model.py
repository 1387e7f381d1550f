"""ctypes loader of the geometry-buffer CPU model (gbuffer_model.c): depth, world position and geometric normal of every pixel of a
frame from its visibility ids.

    import gbuffer_model as gbm
    depth, position, normal = gbm.planes(vis, uniforms, height, grid)
    rec = gbm.pick(pixels, vis, uniforms, height, grid)       # dict: depth (N,), position (N, 3), normal (N, 3), primitive (N,)

`vis` is the frame's visibility (H, W) uint32, primitive id + 1, 0 = background (oracle.render_terrain(..., want_vis=True)); it is
the `primitive` plane itself.
"""
from __future__ import annotations

import numpy as np

import model_support as ms
import occlusion_model as ocm  # noqa: F401  (tests reach these two as gbm.ocm and gbm.om)
import overlay_model as om  # noqa: F401

SIGNATURES = {
    "gbm_planes": "i32(f32*, f32*, f32*, u32*, u32, u32, f32*, f32*, u32, u32, u32)",
    "gbm_pick": "i32(u32*, i32*, u32, u32*, u32, u32, f32*, f32*, u32, u32, u32)",
}


def lib():
    return ms.load("gbuffer_model", SIGNATURES)


def planes(vis, uniforms, height, grid):
    """-> depth (H, W), position (H, W, 3), normal (H, W, 3), float32 (the contract, on the CPU)"""
    _, vis, *scene = ms.frame(None, vis, uniforms, height)
    H, W = vis.shape
    depth, position, normal = np.empty((H, W), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32)
    assert lib().gbm_planes(depth, position, normal, vis, *scene, grid) == 0
    return depth, position, normal


def pick(pixels, vis, uniforms, height, grid):
    """pixels (N, 2) of (x, y) -> what the library's pick returns for them; ValueError if one lies outside the frame"""
    _, vis, *scene = ms.frame(None, vis, uniforms, height)
    px = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
    out = np.zeros((len(px), 8), np.uint32)
    if lib().gbm_pick(out, px, len(px), vis, *scene, grid) != 0:
        raise ValueError("a pixel lies outside the frame")
    f = out.view(np.float32)
    return {"depth": f[:, 0].copy(), "position": f[:, 1:4].copy(), "normal": f[:, 4:7].copy(), "primitive": out[:, 7].copy()}
