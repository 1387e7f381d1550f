"""ctypes loader of the contour CPU model (contour_model.c): the contract of DESIGN.md 4e, producing the records of a contour layer
so that they append to the layers of the overlay / polygon / occlusion models, whose composite draws them.

    import contour_model as cm
    layers = cm.Layers(); layers.points(...); layers.contours(height, grid, uniforms, levels, width_px=1, rgba=(0, 0, 0, 255))
    out = cm.ocm.composite(frame_rgba, vis, uniforms, height, grid, layers)

A contour layer is one feature.  Its records: per segment the segment (flags SEGMENT | DRAPE [| OCCLUDE]), then with round joins a
circle at the segment's p0; y of both ends = lift; size = clamp(width_px, 1, 64) / 2; pad[0] = bits of kb when occluding.
"""
from __future__ import annotations

import numpy as np

import model_support as ms
import occlusion_model as ocm
import overlay_model as om

OVIN = om.OVIN

SIGNATURES = {
    "ctm_heights": "void(f32*, u32, u32, u32, f32*)",
    "ctm_extract": "u64(f32*, u32, f32, f32*, u32, f32, u32, u32, u32, u32, f32, i32, i32, rec48*?, u64)",
}


def lib():
    return ms.load("contour_model", SIGNATURES)


def surface(height, grid):
    """-> (n, n) float32, [j, i] = the displaced height h of grid vertex (i, j): the surface the renderer draws"""
    n = max(int(grid), 2)
    h = np.empty((n, n), np.float32)
    lib().ctm_heights(*ms.texture(height), grid, h)
    return h


def bounds(h):
    """min / max of the finite heights of a surface (what height_bounds() returns)"""
    fin = h[np.isfinite(h)]
    return (float(fin.min()), float(fin.max())) if fin.size else (float("inf"), float("-inf"))


def spacing_of(uniforms):
    return float(max(np.float32(np.asarray(uniforms, np.float32).reshape(44)[36]), np.float32(1e-8)))


def extract(h, spacing, levels, width_px=1.0, rgba=(0, 0, 0, 255), lift=0.0, join="round", occlude=False, depth_bias=ocm.DEPTH_BIAS,
            feature=0, bracket=False):
    """surface h (n, n) -> (records of the layer, number of segments)"""
    h = np.ascontiguousarray(h, np.float32)
    n = h.shape[0]
    assert h.shape == (n, n)
    lv = np.ascontiguousarray(levels, np.float32)
    flags = om.DRAPE | (ocm.OCCLUDE if occlude else 0)
    pad0 = ocm.kb_bits(depth_bias) if occlude else 0
    args = (h, n, float(spacing), lv, len(lv), float(om._half(width_px)), om._rgba_word(rgba), flags, int(feature), pad0,
            float(np.float32(lift)), int(join == "round"), int(bool(bracket)))
    nseg = int(lib().ctm_extract(*args, None, 0))
    recs = np.zeros(nseg * (2 if join == "round" else 1), OVIN)
    assert int(lib().ctm_extract(*args, recs, len(recs))) == nseg
    return recs, nseg


class Layers(ocm.Layers):
    """The occlusion model's layers plus contour layers (which count as point / line layers for set_occlusion)."""

    def contours(self, height, grid, uniforms, levels, width_px=1.0, rgba=(0, 0, 0, 255), lift=0.0, join="round", occlude=False,
                 depth_bias=ocm.DEPTH_BIAS):
        recs, nseg = extract(surface(height, grid), spacing_of(uniforms), levels, width_px, rgba, lift, join, False, depth_bias, self.feature)
        first = len(self.recs)
        self.recs.append(recs)
        self.feature += 1
        self.nsegments = nseg
        return self._occlude(first, occlude, depth_bias)
