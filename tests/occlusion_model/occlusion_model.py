"""ctypes loader of the occlusion CPU model (occlusion_model.c): the polygon model's layers, with point and line layers that can be
hidden behind the terrain.

    import occlusion_model as ocm
    layers = ocm.Layers(); layers.points(xyz, size_px=4, drape=True, occlude=True); layers.lines(paths, occlude=True, depth_bias=0.01)
    out = ocm.composite(frame_rgba, vis, uniforms, height, grid, layers)

`vis` is the frame's visibility (H, W) uint32, primitive id + 1, 0 = background (oracle.render_terrain(..., want_vis=True)).  An
occluding layer's records carry flag 32 and pad[0] = the bits of kb = float32(1) + float32(depth_bias), as
vf_terrain_set_layer_occlusion writes them.
"""
from __future__ import annotations

import numpy as np

import model_support as ms
import overlay_model as om
import polygon_model as pm

OCCLUDE = 32
DEPTH_BIAS = 1e-2                                             # the library's default (include/vf_hip.h VF_OCCLUSION_DEPTH_BIAS)

SIGNATURES = {
    "ocm_composite": "i32(u8*, u32*, u32, u32, f32*, f32*, u32, u32, u32, rec48*, u32, u32, u32*, u32*, u8*, u32*, u32*, f32*)",
    "ocm_terrain_q": "i32(f32*, u8*, u32*, u32, u32, f32*, f32*, u32, u32, u32)",
}


def lib():
    return ms.load("occlusion_model", SIGNATURES)


def kb_bits(depth_bias):
    return int((np.float32(1.0) + np.float32(depth_bias)).view(np.uint32))


class Layers(pm.Layers):
    """Records of point, line and polygon layers in feature order; points and lines may occlude."""

    def __init__(self):
        super().__init__()
        self.ranges = []                                       # per point / line layer: (first, last + 1) into self.recs

    def _occlude(self, first, occlude, depth_bias):
        self.ranges.append((first, len(self.recs)))
        if occlude:
            self.set_occlusion(len(self.ranges) - 1, True, depth_bias)
        return self

    def set_occlusion(self, layer, occlude, depth_bias=DEPTH_BIAS):
        """layer: the index of a point / line layer among those added here (polygon layers are not counted)"""
        a, b = self.ranges[layer]
        for r in self.recs[a:b]:
            if occlude:
                r["flags"] |= OCCLUDE
                r["pad"][:, 0] = kb_bits(depth_bias)
            else:
                r["flags"] &= ~np.uint32(OCCLUDE)
                r["pad"][:, 0] = 0
        return self

    def points(self, xyz, size_px=5.0, rgba=(255, 255, 255, 255), shape="circle", drape=False, occlude=False, depth_bias=DEPTH_BIAS):
        first = len(self.recs)
        super().points(xyz, size_px=size_px, rgba=rgba, shape=shape, drape=drape)
        return self._occlude(first, occlude, depth_bias)

    def lines(self, paths, width_px=2.0, rgba=(255, 255, 255, 255), cap="round", drape=False, occlude=False, depth_bias=DEPTH_BIAS):
        first = len(self.recs)
        super().lines(paths, width_px=width_px, rgba=rgba, cap=cap, drape=drape)
        return self._occlude(first, occlude, depth_bias)

    def polygons(self, polygons, fill_rgba=(255, 255, 255, 255), line_rgba=None, line_width_px=1.0, drape=False):
        n = len(self.ranges)
        super().polygons(polygons, fill_rgba=fill_rgba, line_rgba=line_rgba, line_width_px=line_width_px, drape=drape)
        del self.ranges[n:]                                    # (its outlines went through lines(): not a point / line layer)
        return self


def composite(frame, vis, uniforms, height, grid, layers):
    """frame (H, W, 4) uint8, vis (H, W) uint32 -> a new frame with the layers composited over it (the contract, on the CPU)."""
    out = np.array(frame, np.uint8, copy=True, order="C")
    _, vis, *scene = ms.frame(None, vis, uniforms, height)
    assert vis.shape == out.shape[:2]
    assert lib().ocm_composite(out, vis, *scene, grid, *pm.fill_args(layers)) == 0
    return out


def terrain_q(vis, uniforms, height, grid):
    """-> (Q (H, W) float32: the terrain's interpolated 1/w at each pixel centre, 0 on background; clipped (H, W) bool: the pixel's
    primitive has a vertex outside 0 <= z <= w, so it took the generic path)"""
    _, vis, *scene = ms.frame(None, vis, uniforms, height)
    Q = np.zeros(vis.shape, np.float32)
    clipped = np.zeros(vis.shape, np.uint8)
    assert lib().ocm_terrain_q(Q, clipped, vis, *scene, grid) == 0
    return Q, clipped.astype(bool)
