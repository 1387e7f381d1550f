"""ctypes loader of the haze CPU model (haze_model.c).

    frame, a = hzm.frame(rgba, vis, uniforms, height, grid, density=0.25, start=2.0, falloff=None, ...)
    frame, a, which = hzm.frame(..., want_branch=True)      # which (H, W) int8: -2 background, -1 uniform haze, 0 series, 1 difference
    hzm.det_exp(x); hzm.eye_y(uniforms); hzm.g(eye_y, y, falloff, base); hzm.alpha(d, y, eye_y, **haze)

`rgba` is the frame without haze (H, W, 4) -- the oracle's, or a GPU frame of either shade precision -- and `vis` its visibility
(H, W) uint32; `a` (H, W) float32 is each pixel's opacity, 0 where the pass leaves the pixel as it was.
"""
from __future__ import annotations

import numpy as np

import gbuffer_model as gbm  # noqa: F401  (tests reach it as hzm.gbm)
import model_support as ms

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

SIGNATURES = {
    "hzm_det_exp": "f32(f32)",
    "hzm_det_exp_n": "void(f32*, f32*, u32)",
    "hzm_eye_y": "f32(f32*)",
    "hzm_g_branch": "f32(f32, f32, i32)",
    "hzm_g": "f32(f32, f32, f32, f32)",
    "hzm_g_which": "i32(f32, f32, f32, f32)",
    "hzm_alpha": "f32(f32, f32, f32, f32, f32, f32, f32, f32, u32)",
    "hzm_blend": "void(u8*, u32, f32)",
    "hzm_frame": "i32(u8*, f32*, i8*?, u32*, u32, u32, f32*, f32*, u32, u32, u32, f32, u32, f32, f32, f32, f32, i32)",
}
pack = ms.pack


def lib():
    return ms.load("haze_model", SIGNATURES)


def det_exp(x):
    """the contract's exponential (item 8) of a float or an array of floats in [-87, 16] -> float32"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().hzm_det_exp_n(out, x, x.size)
    return out[()]


def eye_y(uniforms):
    return np.float32(lib().hzm_eye_y(ms.u44(uniforms)))


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
    lib().hzm_blend(px, pack(rgba), float(a))
    return tuple(int(v) for v in px)


def frame(frame_rgba, vis, uniforms, height, grid, density, rgba=DEFAULTS["rgba"], start=0.0, falloff=None, base=0.0, max_opacity=1.0,
          background=False, want_branch=False):
    """frame_rgba: the frame without haze; the other keywords are set_haze's (rgba: the haze colour)
    -> (the hazed frame (H, W, 4) uint8, a (H, W) float32[, which (H, W) int8])"""
    out, vis, *scene = ms.frame(frame_rgba, vis, uniforms, height)
    a = np.empty(vis.shape, np.float32)
    which = np.empty(vis.shape, np.int8) if want_branch else None
    assert lib().hzm_frame(out, a, which, vis, *scene, grid, float(density), pack(rgba), float(start), 0.0 if falloff is None else float(falloff),
                           float(base), float(max_opacity), 1 if background else 0) == 0
    return (out, a, which) if want_branch else (out, a)
