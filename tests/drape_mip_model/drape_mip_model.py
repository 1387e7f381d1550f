"""ctypes loader of the mip-pyramid CPU model (drape_mip_model.c), and the cases the mip tests share.

    import drape_mip_model as dmm
    levels = dmm.pyramid(image)                     # [None, (h1, w1, 4) float16, ...]: level 0 is the image itself
    frame, rewritten = dmm.frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear",
                                 bias=0.0, lit=None, sky=None, strength=0.0, shade_mode=0)
    frame, rewritten, sample = dmm.frame(..., want_sample=True)

As drape_model.frame; `sample` (H, W, 7) float32 holds the drape model's six values and the level of detail (bias included; -inf
where the footprint gives none, +inf for an infinite one) of the pixels written again.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "drape_model"))
import drape_model as drm  # noqa: E402
om = drm.om

# The image the mip tests drape (seeded, opaque and transparent texels, odd and no power of two) and where it lies for each camera:
# chosen so that each camera's rewritten pixels at (257, 131) and bias 0 hold magnified (or top-level) pixels, at least three
# integer levels and blends between two levels in the shares test_drape_mip_model.py asserts.
CASE_SIZE = (1021, 769)
# (a single extent spans some three levels under one camera, so the image lies far beyond the grid and only its middle shows: the
# frame then straddles level 0; the default camera's extent is stretched in z to widen the span)
CASE_EXTENT = {"default": (-5.82, -14.4, 6.18, 17.6), "fill": (-7.76, -7.2, 8.24, 8.8), "near": (-4.85, -4.5, 5.15, 5.5)}


def case_image(seed=29, size=CASE_SIZE):
    """(ih, iw, 4) uint8: blocks of 1, 2, 4 ... 64 texels of one random colour side by side (detail at every level of the pyramid),
    transparent where (ix // 96 + iy // 64) % 4 == 0, alpha 255 on the rest of the left half and random in 1 ... 255 on the right"""
    iw, ih = size
    rng = np.random.default_rng(seed)
    iy, ix = np.meshgrid(np.arange(ih), np.arange(iw), indexing="ij")
    img = np.zeros((ih, iw, 4), np.uint8)
    band = (ix * 7) // iw                                     # seven vertical bands: block sizes 1 ... 64
    for b in range(7):
        s = 1 << b
        colours = rng.integers(0, 256, ((ih + s - 1) // s, (iw + s - 1) // s, 3), dtype=np.uint8)
        m = band == b
        img[m, :3] = colours[iy[m] // s, ix[m] // s]
    alpha = rng.integers(1, 256, (ih, iw), dtype=np.uint8)
    alpha[:, : iw // 2] = 255
    alpha[(ix // 96 + iy // 64) % 4 == 0] = 0
    img[..., 3] = alpha
    return img


def sizes(iw, ih):
    """[(w, h)] of levels 0, 1, ... (the rule of DESIGN.md 4k, stated again in vulkan_forge_amd/_drape.py)"""
    out = [(int(iw), int(ih))]
    while out[-1] != (1, 1):
        w, h = out[-1]
        out.append((max(1, (w + 1) >> 1), max(1, (h + 1) >> 1)))
    return out


_lib = None


def lib():
    global _lib
    if _lib is None:
        T = os.path.dirname(HERE)
        L = om.build_model("libdrmipmodel.so", os.path.join(HERE, "drape_mip_model.c"),
                           [os.path.join(T, "drape_model", "drape_model.c"),
                            os.path.join(T, "ambient_model", "ambient_model.c"), os.path.join(T, "shadow_model", "shadow_model.c"),
                            os.path.join(T, "gbuffer_model", "gbuffer_model.c"), os.path.join(T, "occlusion_model", "occlusion_model.c"),
                            os.path.join(T, "polygon_model", "polygon_model.c"), os.path.join(T, "overlay_model", "overlay_model.c")])
        vp, u32, f, i = C.c_void_p, C.c_uint32, C.c_float, C.c_int
        L.dmm_pyramid.argtypes = [vp, vp, u32, u32]
        L.dmm_pyramid.restype = i
        L.dmm_frame.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, i, vp, u32, u32, vp, vp, f, i, f, vp, vp, f]
        L.dmm_frame.restype = i
        L.dmm_clipped_pixels.argtypes = [vp, u32, u32, vp, vp, u32, u32, u32]
        L.dmm_clipped_pixels.restype = i
        L.dmm_half_bits.argtypes = [f]
        L.dmm_half_bits.restype = C.c_uint16
        L.dmm_half_value.argtypes = [C.c_uint16]
        L.dmm_half_value.restype = f
        _lib = L
    return _lib


_pyramids = {}


def _flat(img):
    """the model's pyramid of a contiguous (ih, iw, 4) image: (flat uint16 buffer, sizes), computed once per image"""
    key = (img.shape, img.tobytes())
    if key not in _pyramids:
        ih, iw = img.shape[:2]
        sz = sizes(iw, ih)
        buf = np.zeros(max(1, 4 * sum(w * h for w, h in sz[1:])), np.uint16)
        assert lib().dmm_pyramid(buf.ctypes.data, img.ctypes.data, iw, ih) == len(sz)
        _pyramids[key] = (buf, sz)
    return _pyramids[key]


def pyramid(image):
    """-> [None, level 1 as (h1, w1, 4) float16, ...]"""
    buf, sz = _flat(drm.rgba8(image))
    out, o = [None], 0
    for w, h in sz[1:]:
        out.append(buf[o:o + 4 * w * h].view(np.float16).reshape(h, w, 4))
        o += 4 * w * h
    return out


def clipped_pixels(vis, uniforms, height, grid):
    """how many covered pixels show a primitive cut by the near or the far plane (the kernels' generic path)"""
    vis = np.ascontiguousarray(vis, np.uint32)
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    n = lib().dmm_clipped_pixels(vis.ctypes.data, vis.shape[1], vis.shape[0], u.ctypes.data, tex.ctypes.data, tex.shape[1], tex.shape[0], grid)
    assert n >= 0
    return n


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear", bias=0.0, lit=None, sky=None,
          strength=0.0, shade_mode=0, want_sample=False):
    """-> (the draped frame (H, W, 4) uint8, rewritten (H, W) bool[, sample (H, W, 7) float32])"""
    vis = np.ascontiguousarray(vis, np.uint32)
    H, W = vis.shape
    out = np.ascontiguousarray(rgba, np.uint8).reshape(H, W, 4).copy()
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    lut = np.ascontiguousarray(lut_rgba8, np.uint8).reshape(1024)
    img = drm.rgba8(image)
    pyr, _ = _flat(img)
    ext = np.ascontiguousarray(drm.FULL_EXTENT if extent is None else extent, np.float32).reshape(4)
    lit = None if lit is None else np.ascontiguousarray(lit, np.float32)
    sky = None if sky is None else np.ascontiguousarray(sky, np.float32)
    mask = np.empty((H, W), np.uint8)
    sample = np.empty((H, W, 7), np.float32) if want_sample else None
    assert filter in ("linear", "nearest")
    assert lib().dmm_frame(out.ctypes.data, mask.ctypes.data, None if sample is None else sample.ctypes.data, vis.ctypes.data, W, H, u.ctypes.data,
                           tex.ctypes.data, tex.shape[1], tex.shape[0], grid, lut.ctypes.data, int(shade_mode), img.ctypes.data, img.shape[1],
                           img.shape[0], pyr.ctypes.data, ext.ctypes.data, float(opacity), 1 if filter == "linear" else 0, float(bias),
                           None if lit is None else lit.ctypes.data, None if sky is None else sky.ctypes.data, float(strength)) == 0
    return (out, mask.astype(bool), sample) if want_sample else (out, mask.astype(bool))
