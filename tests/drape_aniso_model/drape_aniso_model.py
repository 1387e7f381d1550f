"""ctypes loader of the CPU model of anisotropic filtering of the drape's mip sampling (drape_aniso_model.c), and the
cases the anisotropy tests share.

    import drape_aniso_model as dam
    frame, rewritten = dam.frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear",
                                 bias=0.0, max_anisotropy=1, lit=None, sky=None, strength=0.0, shade_mode=0, want_sample=False)
    frame, rewritten, sample = dam.frame(..., want_sample=True)
    ymajor, lod, n = dam.plan(ax, ay, max_anisotropy, bias=0.0)     # items 1 - 4 on the squared axis lengths of a footprint

As drape_mip_model.frame; `sample` (H, W, 10) float32 holds that model's seven values (the level of detail is the plan's), then the
tap count N, the major axis (0 = x, 1 = y) and whether a tap was clamped to the image rectangle, of the pixels written again.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "drape_mip_model"))
import drape_mip_model as dmm  # noqa: E402
drm = dmm.drm
om = drm.om

ANISOTROPIES = (1, 2, 4, 8, 16)
# Where the case image (drape_mip_model.case_image) lies for each camera in the anisotropy tests: each extent is stretched along one
# image axis, found by a scan over half-widths 1.6 ... 48 in x and z, so that the camera's rewritten pixels at (257, 131) and bias 0
# hold one-tap pixels, N = A for every A, counts between, taps at level 0 and blends of two levels in the shares
# test_drape_aniso_model.py asserts (with drape_mip_model.CASE_EXTENT under 2 % of the `default` and `near` pixels are near-isotropic).
# The scenes' height field is noise on a grid far finer than the frame, so the footprints are those of steep sub-pixel primitives:
# the oblique cameras are x-major almost everywhere, and the top-down one supplies the y-major share.
CASE_EXTENT = {"default": (-1.42, -47.7, 1.97, 48.45), "fill": (-8.0, -2.4, 8.5, 2.9), "near": (-47.82, -1.3, 48.37, 2.05)}
# an extent inside the grid, so that taps near its edge leave the image rectangle and are clamped
INTERIOR_EXTENT = (-0.7, -0.5, 0.9, 0.8)

_lib = None


def lib():
    global _lib
    if _lib is None:
        T = os.path.dirname(HERE)
        L = om.build_model("libdranisomodel.so", os.path.join(HERE, "drape_aniso_model.c"),
                           [os.path.join(T, "drape_mip_model", "drape_mip_model.c"), os.path.join(T, "drape_model", "drape_model.c"),
                            os.path.join(T, "ambient_model", "ambient_model.c"), os.path.join(T, "shadow_model", "shadow_model.c"),
                            os.path.join(T, "gbuffer_model", "gbuffer_model.c"), os.path.join(T, "occlusion_model", "occlusion_model.c"),
                            os.path.join(T, "polygon_model", "polygon_model.c"), os.path.join(T, "overlay_model", "overlay_model.c")])
        vp, u32, f, i = C.c_void_p, C.c_uint32, C.c_float, C.c_int
        L.dam_frame.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, i, vp, u32, u32, vp, vp, f, i, f, u32, vp, vp, f]
        L.dam_frame.restype = i
        L.dam_clipped_mask.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, u32]
        L.dam_clipped_mask.restype = i
        L.dam_plan.argtypes = [f, f, u32, f, C.POINTER(i), C.POINTER(f), C.POINTER(u32)]
        L.dam_plan.restype = None
        L.dam_offset.argtypes = [u32, u32]
        L.dam_offset.restype = f
        _lib = L
    return _lib


def plan(ax, ay, max_anisotropy, bias=0.0):
    """items 1 - 4 on the squared lengths of the footprint's screen axes -> (ymajor, lod, N)"""
    ym, lod, n = C.c_int(), C.c_float(), C.c_uint32()
    lib().dam_plan(float(ax), float(ay), int(max_anisotropy), float(bias), C.byref(ym), C.byref(lod), C.byref(n))
    return bool(ym.value), np.float32(lod.value), int(n.value)


def offset(n, i):
    """item 5: the offset of tap i of n along the major axis"""
    return np.float32(lib().dam_offset(int(n), int(i)))


def clipped_mask(vis, uniforms, height, grid):
    """(H, W) bool: the covered pixels that show a primitive cut by the near or the far plane (the kernels' generic path)"""
    vis = np.ascontiguousarray(vis, np.uint32)
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    mask = np.empty(vis.shape, np.uint8)
    assert lib().dam_clipped_mask(mask.ctypes.data, vis.ctypes.data, vis.shape[1], vis.shape[0], u.ctypes.data, tex.ctypes.data, tex.shape[1],
                                  tex.shape[0], grid) == 0
    return mask.astype(bool)


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear", bias=0.0, max_anisotropy=1,
          lit=None, sky=None, strength=0.0, shade_mode=0, want_sample=False):
    """-> (the draped frame (H, W, 4) uint8, rewritten (H, W) bool[, sample (H, W, 10) float32])"""
    assert max_anisotropy in ANISOTROPIES and filter in ("linear", "nearest")
    vis = np.ascontiguousarray(vis, np.uint32)
    H, W = vis.shape
    out = np.ascontiguousarray(rgba, np.uint8).reshape(H, W, 4).copy()
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    lut = np.ascontiguousarray(lut_rgba8, np.uint8).reshape(1024)
    img = drm.rgba8(image)
    pyr, _ = dmm._flat(img)
    ext = np.ascontiguousarray(drm.FULL_EXTENT if extent is None else extent, np.float32).reshape(4)
    lit = None if lit is None else np.ascontiguousarray(lit, np.float32)
    sky = None if sky is None else np.ascontiguousarray(sky, np.float32)
    mask = np.empty((H, W), np.uint8)
    sample = np.empty((H, W, 10), np.float32) if want_sample else None
    assert lib().dam_frame(out.ctypes.data, mask.ctypes.data, None if sample is None else sample.ctypes.data, vis.ctypes.data, W, H, u.ctypes.data,
                           tex.ctypes.data, tex.shape[1], tex.shape[0], grid, lut.ctypes.data, int(shade_mode), img.ctypes.data, img.shape[1],
                           img.shape[0], pyr.ctypes.data, ext.ctypes.data, float(opacity), 1 if filter == "linear" else 0, float(bias),
                           int(max_anisotropy), None if lit is None else lit.ctypes.data, None if sky is None else sky.ctypes.data,
                           float(strength)) == 0
    return (out, mask.astype(bool), sample) if want_sample else (out, mask.astype(bool))
