"""ctypes loader of the geometry-buffer CPU model (gbuffer_model.c): depth, world position and geometric normal of every pixel of a
frame from its visibility ids.

    import gbuffer_model as gbm
    depth, position, normal = gbm.planes(vis, uniforms, height, grid)
    rec = gbm.pick(pixels, vis, uniforms, height, grid)       # dict: depth (N,), position (N, 3), normal (N, 3), primitive (N,)

`vis` is the frame's visibility (H, W) uint32, primitive id + 1, 0 = background (oracle.render_terrain(..., want_vis=True)); it is
the `primitive` plane itself.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "occlusion_model"))
import occlusion_model as ocm  # noqa: E402
om = ocm.om

_lib = None


def lib():
    global _lib
    if _lib is None:
        T = os.path.dirname(HERE)
        L = om.build_model("libgbmodel.so", os.path.join(HERE, "gbuffer_model.c"),
                           [os.path.join(T, "occlusion_model", "occlusion_model.c"), os.path.join(T, "polygon_model", "polygon_model.c"),
                            os.path.join(T, "overlay_model", "overlay_model.c")])
        vp, u32 = C.c_void_p, C.c_uint32
        L.gbm_planes.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, u32, u32, u32]
        L.gbm_planes.restype = C.c_int
        L.gbm_pick.argtypes = [vp, vp, u32, vp, u32, u32, vp, vp, u32, u32, u32]
        L.gbm_pick.restype = C.c_int
        _lib = L
    return _lib


def _frame(vis, uniforms, height):
    vis = np.ascontiguousarray(vis, np.uint32)
    assert vis.ndim == 2
    return vis, np.ascontiguousarray(uniforms, np.float32).reshape(44), np.ascontiguousarray(height, np.float32)


def planes(vis, uniforms, height, grid):
    """-> depth (H, W), position (H, W, 3), normal (H, W, 3), float32 (the contract, on the CPU)"""
    vis, u, tex = _frame(vis, uniforms, height)
    H, W = vis.shape
    depth, position, normal = np.empty((H, W), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32)
    rc = lib().gbm_planes(depth.ctypes.data, position.ctypes.data, normal.ctypes.data, vis.ctypes.data, W, H, u.ctypes.data, tex.ctypes.data,
                          tex.shape[1], tex.shape[0], grid)
    assert rc == 0
    return depth, position, normal


def pick(pixels, vis, uniforms, height, grid):
    """pixels (N, 2) of (x, y) -> what the library's pick returns for them; ValueError if one lies outside the frame"""
    vis, u, tex = _frame(vis, uniforms, height)
    H, W = vis.shape
    px = np.ascontiguousarray(pixels, np.int32).reshape(-1, 2)
    out = np.zeros((len(px), 8), np.uint32)
    rc = lib().gbm_pick(out.ctypes.data, px.ctypes.data, len(px), vis.ctypes.data, W, H, u.ctypes.data, tex.ctypes.data, tex.shape[1],
                        tex.shape[0], grid)
    if rc != 0:
        raise ValueError("a pixel lies outside the frame")
    f = out.view(np.float32)
    return {"depth": f[:, 0].copy(), "position": f[:, 1:4].copy(), "normal": f[:, 4:7].copy(), "primitive": out[:, 7].copy()}
