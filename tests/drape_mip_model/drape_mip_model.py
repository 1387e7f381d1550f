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

import numpy as np

import drape_model as drm
import model_support as ms

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


SIGNATURES = {
    "dmm_pyramid": "i32(u16*, u8*, u32, u32)",
    "dmm_frame": "i32(u8*, u8*, f32*?, u32*, u32, u32, f32*, f32*, u32, u32, u32, u8*, i32, u8*, u32, u32, u16*, f32*, f32, i32, f32, f32*?, f32*?, f32)",
    "dmm_clipped_pixels": "i32(u32*, u32, u32, f32*, f32*, u32, u32, u32)",
    "dmm_half_bits": "u16(f32)",
    "dmm_half_value": "f32(u16)",
}


def lib():
    return ms.load("drape_mip_model", SIGNATURES)


_pyramids = {}


def _flat(img):
    """the model's pyramid of a contiguous (ih, iw, 4) image: (flat uint16 buffer, sizes), computed once per image"""
    key = (img.shape, img.tobytes())
    if key not in _pyramids:
        ih, iw = img.shape[:2]
        sz = sizes(iw, ih)
        buf = np.zeros(max(1, 4 * sum(w * h for w, h in sz[1:])), np.uint16)
        assert lib().dmm_pyramid(buf, img, iw, ih) == len(sz)
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
    n = lib().dmm_clipped_pixels(*ms.frame(None, vis, uniforms, height)[1:], grid)
    assert n >= 0
    return n


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear", bias=0.0, lit=None, sky=None,
          strength=0.0, shade_mode=0, want_sample=False):
    """-> (the draped frame (H, W, 4) uint8, rewritten (H, W) bool[, sample (H, W, 7) float32])"""
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    img = drm.rgba8(image)
    mask = np.empty(vis.shape, np.uint8)
    sample = np.empty(vis.shape + (7,), np.float32) if want_sample else None
    assert filter in ("linear", "nearest")
    assert lib().dmm_frame(out, mask, sample, vis, *scene, grid, ms.lut(lut_rgba8), int(shade_mode), img, img.shape[1], img.shape[0], _flat(img)[0],
                           drm.extent4(extent), float(opacity), 1 if filter == "linear" else 0, float(bias), ms.field(lit), ms.field(sky),
                           float(strength)) == 0
    return (out, mask.astype(bool), sample) if want_sample else (out, mask.astype(bool))
