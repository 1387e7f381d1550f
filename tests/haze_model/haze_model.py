"""ctypes loader of the haze CPU model (haze_model.c).

    frame, a = hzm.frame(rgba, vis, uniforms, height, grid, density=0.25, start=2.0, falloff=None, ...)
    frame, a, which = hzm.frame(..., want_branch=True)      # which (H, W) int8: -2 background, -1 uniform haze, 0 series, 1 difference
    hzm.det_exp(x); hzm.eye_y(uniforms); hzm.g(eye_y, y, falloff, base); hzm.alpha(d, y, eye_y, **haze)

`rgba` is the frame without haze (H, W, 4) -- the oracle's, or a GPU frame of either shade precision -- and `vis` its visibility
(H, W) uint32; `a` (H, W) float32 is each pixel's opacity, 0 where the pass leaves the pixel as it was.
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

DEFAULTS = dict(rgba=(200, 215, 235, 255), start=0.0, falloff=None, base=0.0, max_opacity=1.0, background=False)
SERIES_BELOW = 0.5            # |s| below this: the series branch of g (HZ_SERIES_BELOW)
# The GPU tests' settings, per test camera (overlay_scenes.CAMERAS).  The cameras see view depths of 3.8 to 9.1 (default), 2.0 to 4.0
# (fill) and 1.0 to 2.4 (near), ranges that do not overlap enough for one `start` to cut all three: each camera's start is near the
# first quartile of its depths, so about a quarter of its covered pixels are left untouched and the rest have 0 < a < max_opacity
# (tests/test_haze_model.py asserts between 10 % and 90 %).  The eyes stand at y = 2.0, 2.2 and 0.6 over ground of |y| < 0.8: falloff
# 0.3 puts the first two cameras on the difference branch of g and the near camera on both branches, falloff 4 puts the first two on
# both, falloff 50 all three on the series.
SCENE_PARAMS = {"default": dict(density=0.6, start=4.5), "fill": dict(density=0.6, start=2.5), "near": dict(density=0.6, start=1.1)}
SCENE_FALLOFFS = (0.3, 4.0, 50.0)
SCENE_BASE = 0.2

_lib = None


def lib():
    global _lib
    if _lib is None:
        T = os.path.dirname(HERE)
        L = om.build_model("libhzmodel.so", os.path.join(HERE, "haze_model.c"),
                           [os.path.join(T, "gbuffer_model", "gbuffer_model.c"), os.path.join(T, "occlusion_model", "occlusion_model.c"),
                            os.path.join(T, "polygon_model", "polygon_model.c"), os.path.join(T, "overlay_model", "overlay_model.c")])
        vp, u32, f, i = C.c_void_p, C.c_uint32, C.c_float, C.c_int
        L.hzm_det_exp.argtypes = [f]
        L.hzm_det_exp.restype = f
        L.hzm_det_exp_n.argtypes = [vp, vp, u32]
        L.hzm_det_exp_n.restype = None
        L.hzm_eye_y.argtypes = [vp]
        L.hzm_eye_y.restype = f
        L.hzm_g_branch.argtypes = [f, f, i]
        L.hzm_g_branch.restype = f
        L.hzm_g.argtypes = [f, f, f, f]
        L.hzm_g.restype = f
        L.hzm_g_which.argtypes = [f, f, f, f]
        L.hzm_g_which.restype = i
        L.hzm_alpha.argtypes = [f, f, f, f, f, f, f, f, u32]
        L.hzm_alpha.restype = f
        L.hzm_blend.argtypes = [vp, u32, f]
        L.hzm_blend.restype = None
        L.hzm_frame.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, u32, u32, u32, f, u32, f, f, f, f, i]
        L.hzm_frame.restype = i
        _lib = L
    return _lib


def pack(rgba):
    r, g, b, a = (int(v) for v in rgba)
    return r | g << 8 | b << 16 | a << 24


def det_exp(x):
    """the contract's exponential (item 8) of a float or an array of floats in [-87, 16] -> float32"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().hzm_det_exp_n(out.ctypes.data, x.ctypes.data, x.size)
    return out[()]


def eye_y(uniforms):
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    return np.float32(lib().hzm_eye_y(u.ctypes.data))


def g_branch(k_e, k_p, branch=-1):
    """the height factor from the two clamped heights in units of the falloff; branch 0: the series, 1: the difference, -1: the contract's choice"""
    return np.float32(lib().hzm_g_branch(float(k_e), float(k_p), int(branch)))


def g(eye, y, falloff, base=0.0):
    return np.float32(lib().hzm_g(float(eye), float(y), 0.0 if falloff is None else float(falloff), float(base)))


def alpha(d, y, eye, density, rgba=DEFAULTS["rgba"], start=0.0, falloff=None, base=0.0, max_opacity=1.0):
    """the opacity of a surface point at view depth d and height y (items 1, 2, 5); 0: the pixel is untouched"""
    return np.float32(lib().hzm_alpha(float(d), float(y), float(eye), float(density), float(start), 0.0 if falloff is None else float(falloff),
                                      float(base), float(max_opacity), int(rgba[3])))


def blend(pixel_rgb, rgba, a):
    """three colour bytes under the haze colour with opacity a (item 6) -> three bytes"""
    px = np.array(list(pixel_rgb)[:3], np.uint8)
    lib().hzm_blend(px.ctypes.data, pack(rgba), float(a))
    return tuple(int(v) for v in px)


def frame(frame_rgba, vis, uniforms, height, grid, density, rgba=DEFAULTS["rgba"], start=0.0, falloff=None, base=0.0, max_opacity=1.0,
          background=False, want_branch=False):
    """frame_rgba: the frame without haze; the other keywords are set_haze's (rgba: the haze colour)
    -> (the hazed frame (H, W, 4) uint8, a (H, W) float32[, which (H, W) int8])"""
    colour = rgba
    vis = np.ascontiguousarray(vis, np.uint32)
    H, W = vis.shape
    out = np.ascontiguousarray(frame_rgba, np.uint8).reshape(H, W, 4).copy()
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    a = np.empty((H, W), np.float32)
    which = np.empty((H, W), np.int8) if want_branch else None
    assert lib().hzm_frame(out.ctypes.data, a.ctypes.data, which.ctypes.data if want_branch else None, vis.ctypes.data, W, H, u.ctypes.data,
                           tex.ctypes.data, tex.shape[1], tex.shape[0], grid, float(density), pack(colour), float(start),
                           0.0 if falloff is None else float(falloff), float(base), float(max_opacity), 1 if background else 0) == 0
    return (out, a, which) if want_branch else (out, a)
