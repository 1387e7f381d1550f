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

import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "contour_model"))
import contour_model as cm  # noqa: E402
ocm = cm.ocm
om = cm.om

HAZE = 64
HAZE_RGBA = (200, 215, 235, 255)                              # the library's default haze colour (include/vf_hip.h VF_HAZE_RGBA)

_lib = None


def lib():
    global _lib
    if _lib is None:
        T = os.path.dirname(HERE)
        L = om.build_model("libohmodel.so", os.path.join(HERE, "overlay_haze_model.c"),
                           [os.path.join(T, "occlusion_model", "occlusion_model.c"), os.path.join(T, "polygon_model", "polygon_model.c"),
                            os.path.join(T, "overlay_model", "overlay_model.c")])
        vp, u32, i32, f, i = C.c_void_p, C.c_uint32, C.c_int32, C.c_float, C.c_int
        L.ohm_composite.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, u32, u32, vp, vp, vp, vp, vp, vp, f, u32, f, f, f, f, vp, vp, vp]
        L.ohm_composite.restype = i
        L.ohm_alpha_n.argtypes = [vp, vp, vp, u32, f, f, f, f, f, f, u32]
        L.ohm_alpha_n.restype = None
        L.ohm_probe.argtypes = [vp, u32, u32, vp, vp, u32, u32, u32, vp, i32, i32, f, u32, f, f, f, f]
        L.ohm_probe.restype = i
        _lib = L
    return _lib


def haze_words(haze):
    """set_haze's keywords -> (density, packed colour, start, falloff (0: uniform), base, max_opacity); no haze: density 0"""
    if haze is None or not haze.get("enabled", True):
        haze = dict(density=0.0)
    r, g, b, a = (int(v) for v in haze.get("rgba", HAZE_RGBA))
    fo = haze.get("falloff")
    return (float(haze["density"]), r | g << 8 | b << 16 | a << 24, float(haze.get("start", 0.0)), 0.0 if fo is None else float(fo),
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
    H, W = out.shape[:2]
    vis = np.ascontiguousarray(vis, np.uint32)
    assert vis.shape == (H, W)
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    recs = np.ascontiguousarray(layers.array())
    fills = getattr(layers, "fills", [])
    feat = np.array([f[0] for f in fills], np.uint32)
    cols = np.array([f[1] for f in fills], np.uint32)
    drape = np.array([f[2] for f in fills], np.uint8)
    rings = [r for f in fills for r in f[3]]
    fr = np.zeros(len(fills) + 1, np.uint32)
    fr[1:] = np.cumsum([len(f[3]) for f in fills])
    offs, xyz = ocm.pm._pack(rings)
    ah = np.zeros((H, W), np.float32)
    touch = np.zeros((H, W), np.uint8)
    counts = np.zeros(3, np.uint64)
    rc = lib().ohm_composite(out.ctypes.data, vis.ctypes.data, W, H, u.ctypes.data, tex.ctypes.data, tex.shape[1], tex.shape[0], grid,
                             recs.ctypes.data, len(recs), len(fills), feat.ctypes.data, cols.ctypes.data, drape.ctypes.data,
                             fr.ctypes.data, offs.ctypes.data, xyz.ctypes.data, *haze_words(haze), ah.ctypes.data, touch.ctypes.data, counts.ctypes.data)
    assert rc == 0
    if want_counts:
        return out, tuple(int(v) for v in counts)
    return (out, ah, touch.astype(bool)) if want_planes else out


def alpha(d, y, eye, density, rgba=HAZE_RGBA, start=0.0, falloff=None, base=0.0, max_opacity=1.0, **_):
    """the model's restatement of the haze opacity of arrays of depths and heights -> float32 array"""
    d = np.ascontiguousarray(d, np.float32)
    y = np.ascontiguousarray(y, np.float32)
    assert d.shape == y.shape
    out = np.empty_like(d)
    lib().ohm_alpha_n(out.ctypes.data, d.ctypes.data, y.ctypes.data, d.size, float(eye), float(density), float(start),
                      0.0 if falloff is None else float(falloff), float(base), float(max_opacity), int(rgba[3]))
    return out


def probe(W, H, uniforms, height, grid, record, px, py, haze):
    """one record (an OVIN row) at pixel (px, py) -> dict(cover, d, y, t, ah, rw_a, rw_b, y_a, y_b): the ends after clipping"""
    u = np.ascontiguousarray(uniforms, np.float32).reshape(44)
    tex = np.ascontiguousarray(height, np.float32)
    rec = np.ascontiguousarray(np.asarray(record, om.OVIN).reshape(1))
    out = np.zeros(9, np.float32)
    assert lib().ohm_probe(out.ctypes.data, W, H, u.ctypes.data, tex.ctypes.data, tex.shape[1], tex.shape[0], grid, rec.ctypes.data, int(px), int(py),
                           *haze_words(haze)) == 0
    return dict(zip(("cover", "d", "y", "t", "ah", "rw_a", "rw_b", "y_a", "y_b"), out))
