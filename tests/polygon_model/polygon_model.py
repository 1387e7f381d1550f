"""ctypes loader of the polygon fill CPU model (polygon_model.c), with layers that mix polygons, points and lines.

    import polygon_model as pm
    layers = pm.Layers(); layers.points(xyz, size_px=4); layers.polygons(polys, fill_rgba=(0, 90, 255, 160), line_rgba=(0, 0, 0, 255))
    out = pm.composite(frame_rgba, uniforms, height, grid, layers)

A polygon layer is what include/vf_hip.h documents for vf_terrain_add_polygons: every polygon's fill (one feature each, in order),
then the outline of every ring as its own polyline feature -- the ring closed back to its first vertex, round caps.  Rings are used
as given (vulkan_forge.pack_polygons does the duplicate and closing-vertex removal).
"""
from __future__ import annotations

import numpy as np

import model_support as ms
import overlay_model as om

SIGNATURES = {
    "pgm_composite": "i32(u8*, u32, u32, f32*, f32*, u32, u32, u32, rec48*, u32, u32, u32*, u32*, u8*, u32*, u32*, f32*)",
    "pgm_fill_coverage": "i32(f32*, u32, u32, f32*, f32*, u32, u32, u32, u32, u32*, f32*, i32)",
    "pgm_ring_edges": "i32(f32*, u32, u32, f32*, f32*, u32, u32, u32, f32*, u32, i32)",
}


def lib():
    return ms.load("polygon_model", SIGNATURES)


def _rings(poly):
    """a polygon (one (k, 3) ring or a sequence of rings) -> list of (k, 3) float32 arrays"""
    if isinstance(poly, np.ndarray) and poly.ndim == 2:
        poly = [poly]
    return [np.ascontiguousarray(r, np.float32).reshape(-1, 3) for r in poly]


class Layers(om.Layers):
    """Primitive records of points and lines (overlay model) plus fill features, in one feature order."""

    def __init__(self):
        super().__init__()
        self.fills = []                                        # (feature, rgba word, drape, rings)

    def polygons(self, polygons, fill_rgba=(255, 255, 255, 255), line_rgba=None, line_width_px=1.0, drape=False):
        polys = [_rings(p) for p in polygons]
        if fill_rgba is not None:
            cols = np.asarray(fill_rgba, np.uint8)
            cols = np.broadcast_to(cols, (len(polys), 4)) if cols.ndim == 1 else cols
            for p, c in zip(polys, cols):
                self.fills.append((self.feature, om._rgba_word(c), bool(drape), p))
                self.feature += 1
        if line_rgba is not None:
            closed = [np.concatenate([r, r[:1]]) for p in polys for r in p]
            self.lines(closed, width_px=line_width_px, rgba=line_rgba, cap="round", drape=drape)
        return self


def _pack(rings):
    offs = np.zeros(len(rings) + 1, np.uint32)
    offs[1:] = np.cumsum([len(r) for r in rings])
    xyz = np.ascontiguousarray(np.concatenate(rings) if rings else np.zeros((0, 3), np.float32), np.float32)
    return offs, xyz


def fill_args(layers):
    """the records and the fill features of `layers` as the composites of this, the occlusion and the hazed-overlay model take them:
    (records, their count, the number of fills, their features, colours, drape flags, ring ranges, the rings' vertex offsets, xyz)"""
    recs = np.ascontiguousarray(layers.array())
    fills = getattr(layers, "fills", [])
    feat = np.array([f[0] for f in fills], np.uint32)
    cols = np.array([f[1] for f in fills], np.uint32)
    drape = np.array([f[2] for f in fills], np.uint8)
    fr = np.zeros(len(fills) + 1, np.uint32)
    fr[1:] = np.cumsum([len(f[3]) for f in fills])
    return (recs, len(recs), len(fills), feat, cols, drape, fr, *_pack([r for f in fills for r in f[3]]))


def composite(frame, uniforms, height, grid, layers):
    """frame (H, W, 4) uint8 -> a new frame with the layers composited over it (the contract, on the CPU)."""
    out = np.array(frame, np.uint8, copy=True, order="C")
    H, W = out.shape[:2]
    assert lib().pgm_composite(out, W, H, ms.u44(uniforms), *ms.texture(height), grid, *fill_args(layers)) == 0
    return out


def fill_coverage(W, H, uniforms, height, grid, polygon, drape=False):
    """(H, W) float32 coverage of one polygon's fill"""
    cov = np.zeros((H, W), np.float32)
    rings = _rings(polygon)
    assert lib().pgm_fill_coverage(cov, W, H, ms.u44(uniforms), *ms.texture(height), grid, len(rings), *_pack(rings), int(bool(drape))) == 0
    return cov


EDGE = ("x0", "y0", "ex", "ey", "il2", "s", "xmin", "xmax", "ymin", "ymax")


def ring_edges(W, H, uniforms, height, grid, ring, drape=False):
    """(n, 10) float32: one ring's screen edge set after near-plane clipping, columns EDGE"""
    ring = np.ascontiguousarray(ring, np.float32).reshape(-1, 3)
    out = np.zeros((2 * len(ring), 10), np.float32)
    n = lib().pgm_ring_edges(out, W, H, ms.u44(uniforms), *ms.texture(height), grid, ring, len(ring), int(bool(drape)))
    assert n >= 0
    return out[:n]
