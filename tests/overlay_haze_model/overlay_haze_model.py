"""ctypes loader of the hazed-overlay CPU model (overlay_haze_model.c): the contour model's layers (points, lines, polygons, contours,
occlusion), whose point, line and contour layers can take the atmospheric haze.

    import overlay_haze_model as ohm
    layers = ohm.Layers(); layers.points(xyz, size_px=4, drape=True, haze=True); layers.lines(paths, haze=True, occlude=True)
    out = ohm.composite(frame_rgba, vis, uniforms, height, grid, layers, haze=dict(density=0.6, start=4.5, falloff=4.0, base=0.2))
    out, ah, touch = ohm.composite(..., want_planes=True)

`haze` holds set_haze's keywords (density, rgba, start, falloff, base, max_opacity; background and enabled=True are accepted and play
no part); None, enabled=False or density 0: no haze, the frame is the occlusion model's.  A hazed layer's records carry flag 64, as
vf_terrain_set_layer_haze writes it.  `ah` (H, W) float32 is the haze opacity of the last hazed feature that covers each pixel,
`touch` (H, W) bool where a hazed feature covers the pixel.
"""
from __future__ import annotations

import numpy as np

import contour_model as cm
import model_support as ms
import occlusion_model as ocm  # noqa: F401  (tests reach it as ohm.ocm)
import overlay_model as om
import polygon_model as pm

HAZE = 64
HAZE_RGBA = (200, 215, 235, 255)                              # the library's default haze colour (include/vf_hip.h VF_HAZE_RGBA)

SIGNATURES = {
    "ohm_composite": "i32(u8*, u32*, u32, u32, f32*, f32*, u32, u32, u32, rec48*, u32, u32, u32*, u32*, u8*, u32*, u32*, f32*, f32, u32, f32, f32, f32, f32, f32*, u8*, u64*)",
    "ohm_alpha_n": "void(f32*, f32*, f32*, u32, f32, f32, f32, f32, f32, f32, u32)",
    "ohm_probe": "i32(f32*, u32, u32, f32*, f32*, u32, u32, u32, rec48*, i32, i32, f32, u32, f32, f32, f32, f32)",
}


def lib():
    return ms.load("overlay_haze_model", SIGNATURES)


def haze_words(haze):
    """set_haze's keywords -> (density, packed colour, start, falloff (0: uniform), base, max_opacity); no haze: density 0"""
    if haze is None or not haze.get("enabled", True):
        haze = dict(density=0.0)
    fo = haze.get("falloff")
    return (float(haze["density"]), ms.pack(haze.get("rgba", HAZE_RGBA)), float(haze.get("start", 0.0)), 0.0 if fo is None else float(fo),
            float(haze.get("base", 0.0)), float(haze.get("max_opacity", 1.0)))


class Layers(cm.Layers):
    """The contour model's layers; point, line and contour layers may take the haze."""

    def _haze(self, haze):
        if haze:
            self.set_haze(len(self.ranges) - 1, True)
        return self

    def set_haze(self, layer, on=True):
        """layer: the index of a point / line / contour layer among those added here (polygon layers are not counted)"""
        a, b = self.ranges[layer]
        for r in self.recs[a:b]:
            if on:
                r["flags"] |= np.uint32(HAZE)
            else:
                r["flags"] &= ~np.uint32(HAZE)
        return self

    def layer_haze(self, layer):
        a, b = self.ranges[layer]
        return any((r["flags"] & HAZE).any() for r in self.recs[a:b])

    def points(self, xyz, haze=False, **kw):
        super().points(xyz, **kw)
        return self._haze(haze)

    def lines(self, paths, haze=False, **kw):
        super().lines(paths, **kw)
        return self._haze(haze)

    def contours(self, height, grid, uniforms, levels, haze=False, **kw):
        super().contours(height, grid, uniforms, levels, **kw)
        return self._haze(haze)


def composite(frame, vis, uniforms, height, grid, layers, haze=None, want_planes=False, want_counts=False):
    """frame (H, W, 4) uint8, vis (H, W) uint32 -> a new frame with the layers composited over it under `haze` (the contract, on the
    CPU)[, ah (H, W) float32, touch (H, W) bool]; want_counts: -> (frame, (pairs, middle, clear)): the (hazed feature, covered pixel)
    pairs, those with 0 < S.ah < max_opacity, those with S.ah == 0"""
    out = np.array(frame, np.uint8, copy=True, order="C")
    _, vis, *scene = ms.frame(None, vis, uniforms, height)
    assert vis.shape == out.shape[:2]
    ah = np.zeros(vis.shape, np.float32)
    touch = np.zeros(vis.shape, np.uint8)
    counts = np.zeros(3, np.uint64)
    assert lib().ohm_composite(out, vis, *scene, grid, *pm.fill_args(layers), *haze_words(haze), ah, touch, counts) == 0
    if want_counts:
        return out, tuple(int(v) for v in counts)
    return (out, ah, touch.astype(bool)) if want_planes else out


def alpha(d, y, eye, density, rgba=HAZE_RGBA, start=0.0, falloff=None, base=0.0, max_opacity=1.0, **_):
    """the model's restatement of the haze opacity of arrays of depths and heights -> float32 array"""
    d = np.ascontiguousarray(d, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    assert d.shape == y.shape
    out = np.empty_like(d)
    lib().ohm_alpha_n(out, d, y, d.size, float(eye), float(density), float(start), 0.0 if falloff is None else float(falloff), float(base),
                      float(max_opacity), int(rgba[3]))
    return out


def probe(W, H, uniforms, height, grid, record, px, py, haze):
    """one record (an OVIN row) at pixel (px, py) -> dict(cover, d, y, t, ah, rw_a, rw_b, y_a, y_b): the ends after clipping"""
    rec = np.ascontiguousarray(np.asarray(record, om.OVIN).reshape(1))
    out = np.zeros(9, np.float32)
    assert lib().ohm_probe(out, W, H, ms.u44(uniforms), *ms.texture(height), grid, rec, int(px), int(py), *haze_words(haze)) == 0
    return dict(zip(("cover", "d", "y", "t", "ah", "rw_a", "rw_b", "y_a", "y_b"), out))
