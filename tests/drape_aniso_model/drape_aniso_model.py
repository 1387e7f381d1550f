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

import numpy as np

import drape_mip_model as dmm
import drape_model as drm
import model_support as ms

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

SIGNATURES = {
    "dam_frame": "i32(u8*, u8*, f32*?, u32*, u32, u32, f32*, f32*, u32, u32, u32, u8*, i32, u8*, u32, u32, u16*, f32*, f32, i32, f32, u32, f32*?, f32*?, f32)",
    "dam_clipped_mask": "i32(u8*, u32*, u32, u32, f32*, f32*, u32, u32, u32)",
    "dam_plan": "void(f32, f32, u32, f32, i32*, f32*, u32*)",
    "dam_offset": "f32(u32, u32)",
}


def lib():
    return ms.load("drape_aniso_model", SIGNATURES)


def plan(ax, ay, max_anisotropy, bias=0.0):
    """items 1 - 4 on the squared lengths of the footprint's screen axes -> (ymajor, lod, N)"""
    ym, lod, n = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.uint32)
    lib().dam_plan(float(ax), float(ay), int(max_anisotropy), float(bias), ym, lod, n)
    return bool(ym[0]), lod[0], int(n[0])


def offset(n, i):
    """item 5: the offset of tap i of n along the major axis"""
    return np.float32(lib().dam_offset(int(n), int(i)))


def clipped_mask(vis, uniforms, height, grid):
    """(H, W) bool: the covered pixels that show a primitive cut by the near or the far plane (the kernels' generic path)"""
    _, vis, *scene = ms.frame(None, vis, uniforms, height)
    mask = np.empty(vis.shape, np.uint8)
    assert lib().dam_clipped_mask(mask, vis, *scene, grid) == 0
    return mask.astype(bool)


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear", bias=0.0, max_anisotropy=1,
          lit=None, sky=None, strength=0.0, shade_mode=0, want_sample=False):
    """-> (the draped frame (H, W, 4) uint8, rewritten (H, W) bool[, sample (H, W, 10) float32])"""
    assert max_anisotropy in ANISOTROPIES and filter in ("linear", "nearest")
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    img = drm.rgba8(image)
    mask = np.empty(vis.shape, np.uint8)
    sample = np.empty(vis.shape + (10,), np.float32) if want_sample else None
    assert lib().dam_frame(out, mask, sample, vis, *scene, grid, ms.lut(lut_rgba8), int(shade_mode), img, img.shape[1], img.shape[0],
                           dmm._flat(img)[0], drm.extent4(extent), float(opacity), 1 if filter == "linear" else 0, float(bias),
                           int(max_anisotropy), ms.field(lit), ms.field(sky), float(strength)) == 0
    return (out, mask.astype(bool), sample) if want_sample else (out, mask.astype(bool))
