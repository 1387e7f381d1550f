"""ctypes loader of the overlay CPU model (overlay_model.c) and the layer packing it shares with the library's contract.

    import overlay_model as om
    layers = om.Layers(); layers.points(xyz, size_px=4, rgba=(255, 0, 0, 255)); layers.lines(paths, width_px=2, cap="round")
    out = om.composite(frame_rgba, uniforms, height, grid, layers)

The packing below is what include/vf_hip.h documents for vf_terrain_add_points / _add_lines: a point is one circle or square of
radius clamp(size_px, 1, 64) / 2; a path is its segments plus discs (radius clamp(width_px, 1, 64) / 2) at interior vertices and,
for round caps, at both ends; square caps extend the first and last segment by the half width.  Features are numbered in order.
"""
from __future__ import annotations

import numpy as np

import model_support as ms

OVIN = np.dtype([("p0", "<f4", (3,)), ("p1", "<f4", (3,)), ("size", "<f4"), ("flags", "<u4"), ("rgba", "<u4"), ("feature", "<u4"),
                 ("pad", "<u4", (2,))])
assert OVIN.itemsize == 48
CIRCLE, SQUARE, SEGMENT, DRAPE, EXT0, EXT1 = 0, 1, 2, 4, 8, 16
SHAPES = {"circle": CIRCLE, "square": SQUARE}
CAPS = ("butt", "square", "round")

SIGNATURES = {
    "ovm_composite": "i32(u8*, u32, u32, f32*, f32*, u32, u32, u32, rec48*, u32)",
    "ovm_decode": "f32(u32)",
    "ovm_encode": "u32(f32)",
    "ovm_drape": "f32(f32*, f32*, u32, u32, u32, f32, f32)",
    "ovm_vertex_height": "f32(f32*, u32, u32, u32, u32, u32)",
}


def lib():
    return ms.load("overlay_model", SIGNATURES)


def _half(v):
    return np.float32(min(max(np.float32(v), np.float32(1.0)), np.float32(64.0))) * np.float32(0.5)


_rgba_word = ms.pack


class Layers:
    """Primitive records of a sequence of layers, in feature order (as the library builds them)."""

    def __init__(self):
        self.recs = []
        self.feature = 0

    def points(self, xyz, size_px=5.0, rgba=(255, 255, 255, 255), shape="circle", drape=False):
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        n = len(xyz)
        sizes = np.broadcast_to(np.asarray(size_px, np.float32), (n,))
        cols = np.asarray(rgba, np.uint8)
        cols = np.broadcast_to(cols, (n, 4)) if cols.ndim == 1 else cols
        keep = np.isfinite(xyz).all(axis=1)
        xyz, sizes, cols = xyz[keep], sizes[keep], cols[keep]
        m = len(xyz)
        r = np.zeros(m, OVIN)
        r["p0"] = xyz
        r["p1"] = xyz
        r["size"] = np.minimum(np.maximum(sizes, np.float32(1)), np.float32(64)) * np.float32(0.5)
        r["flags"] = SHAPES[shape] | (DRAPE if drape else 0)
        c = cols.astype(np.uint32)
        r["rgba"] = c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)
        r["feature"] = self.feature + np.arange(m, dtype=np.uint32)
        self.feature += m
        self.recs.append(r)
        return self

    def lines(self, paths, width_px=2.0, rgba=(255, 255, 255, 255), cap="round", drape=False):
        """paths: a sequence of (k, 3) arrays (used as given: no duplicate removal here)"""
        hw = _half(width_px)
        word = _rgba_word(rgba)
        base = DRAPE if drape else 0
        out = []
        for p in paths:
            p = np.asarray(p, np.float32).reshape(-1, 3)
            m = len(p)
            for v in range(m):
                if (0 < v < m - 1) or cap == "round":
                    out.append(((p[v], p[v]), CIRCLE | base))
                if v + 1 < m:
                    fl = SEGMENT | base
                    if cap == "square" and v == 0:
                        fl |= EXT0
                    if cap == "square" and v + 2 == m:
                        fl |= EXT1
                    out.append(((p[v], p[v + 1]), fl))
            r = np.zeros(len(out), OVIN)
            for k, ((a, b), fl) in enumerate(out):
                r[k]["p0"], r[k]["p1"], r[k]["flags"] = a, b, fl
            r["size"] = hw
            r["rgba"] = word
            r["feature"] = self.feature
            self.feature += 1
            self.recs.append(r)
            out = []
        return self

    def array(self):
        return np.concatenate(self.recs) if self.recs else np.zeros(0, OVIN)


def composite(frame, uniforms, height, grid, layers):
    """frame (H, W, 4) uint8 -> a new frame with the layers composited over it (the contract, on the CPU)."""
    out = np.array(frame, np.uint8, copy=True, order="C")
    H, W = out.shape[:2]
    recs = np.ascontiguousarray(layers.array() if isinstance(layers, Layers) else layers)
    assert lib().ovm_composite(out, W, H, ms.u44(uniforms), *ms.texture(height), grid, recs, len(recs)) == 0
    return out


def decode(k):
    return lib().ovm_decode(int(k))


def encode(c):
    return lib().ovm_encode(float(c))


def drape(uniforms, height, grid, x, z):
    return lib().ovm_drape(ms.u44(uniforms), *ms.texture(height), grid, float(x), float(z))


def vertex_height(height, grid, i, j):
    return lib().ovm_vertex_height(*ms.texture(height), grid, i, j)
