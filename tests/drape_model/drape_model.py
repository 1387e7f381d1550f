"""ctypes loader of the draped-image CPU model (drape_model.c), and the image the drape tests share.

    import drape_model as drm
    frame, rewritten = drm.frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear",
                                 lit=None, sky=None, strength=0.0, shade_mode=0)
    frame, rewritten, sample = drm.frame(..., want_sample=True)

`rgba` is the plain frame (H, W, 4) and `vis` its visibility (H, W) uint32 (oracle.render_terrain); `image` (ih, iw, 4) or (ih, iw, 3)
uint8; `lit` / `sky` the shadow and sky-view fields when those features are on; `rewritten` marks the pixels the shade pass writes
again and `sample` (H, W, 6) float32 holds their filtered premultiplied (r, g, b, a) and the lit and amb they were shaded with.
"""
from __future__ import annotations

import numpy as np

import ambient_model as abm  # noqa: F401  (tests reach these two as drm.abm and drm.shm)
import model_support as ms
import shadow_model as shm  # noqa: F401

FULL_EXTENT = (-1.5, -1.5, 1.5, 1.5)
# The tests' image and where it lies: 37 x 53 texels (iw x ih) over a part of the grid and beyond its z edge (the grid ends at 1.5).
IMAGE_SIZE = (37, 53)
EXTENT = (-1.1, -0.9, 1.3, 1.6)
# the same per camera (test_drape_model.py asserts that between 10 % and 90 % of each camera's covered pixels are written again)
SCENE_EXTENT = {"default": EXTENT, "fill": EXTENT, "near": EXTENT}


def image(seed=11, size=IMAGE_SIZE):
    """(ih, iw, 4) uint8 from a seeded generator: alpha 0 where (ix // 6 + iy // 6) % 3 == 0, elsewhere a random value in 1 ... 255"""
    iw, ih = size
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (ih, iw, 4), dtype=np.uint8)
    img[..., 3] = rng.integers(1, 256, (ih, iw), dtype=np.uint8)
    iy, ix = np.meshgrid(np.arange(ih), np.arange(iw), indexing="ij")
    img[(ix // 6 + iy // 6) % 3 == 0, 3] = 0
    return img


def opaque_image(size, seed=3):
    """(ih, iw, 4) uint8, random colours, alpha 255"""
    iw, ih = size
    img = np.random.default_rng(seed).integers(0, 256, (ih, iw, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


SIGNATURES = {
    "drm_frame": "i32(u8*, u8*, f32*?, u32*, u32, u32, f32*, f32*, u32, u32, u32, u8*, i32, u8*, u32, u32, f32*, f32, i32, f32*?, f32*?, f32)",
}


def lib():
    return ms.load("drape_model", SIGNATURES)


def rgba8(img):
    """(ih, iw, 3 | 4) uint8 -> contiguous (ih, iw, 4): RGB gets alpha 255"""
    img = np.asarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] in (3, 4)
    if img.shape[2] == 3:
        img = np.concatenate([img, np.full(img.shape[:2] + (1,), 255, np.uint8)], axis=2)
    return np.ascontiguousarray(img)


def extent4(extent):
    """the image's (x0, z0, x1, z1) as four float32; None: the whole grid"""
    return np.ascontiguousarray(FULL_EXTENT if extent is None else extent, np.float32).reshape(4)


def frame(rgba, vis, uniforms, height, grid, lut_rgba8, image, extent=None, opacity=1.0, filter="linear", lit=None, sky=None, strength=0.0,
          shade_mode=0, want_sample=False):
    """-> (the draped frame (H, W, 4) uint8, rewritten (H, W) bool[, sample (H, W, 6) float32])"""
    out, vis, *scene = ms.frame(rgba, vis, uniforms, height)
    img = rgba8(image)
    mask = np.empty(vis.shape, np.uint8)
    sample = np.empty(vis.shape + (6,), np.float32) if want_sample else None
    assert filter in ("linear", "nearest")
    assert lib().drm_frame(out, mask, sample, vis, *scene, grid, ms.lut(lut_rgba8), int(shade_mode), img, img.shape[1], img.shape[0],
                           extent4(extent), float(opacity), 1 if filter == "linear" else 0, ms.field(lit), ms.field(sky), float(strength)) == 0
    return (out, mask.astype(bool), sample) if want_sample else (out, mask.astype(bool))
