"""The cumulative viewshed's CPU model: numpy over the viewshed model (tests/viewshed_model).

    total = cvm.sum_heights(h, vertices, exag=1.0, rc=None, eye_height=..., ...)       # (n, n) uint32: the sum of q over the observers
    count = cvm.count(total)                                                           # (n, n) float32 in [0, N]
    count, vertices = cvm.field(uniforms, height, grid, observers, radius=None, ...)   # the renderer's own surface
    frame, s = cvm.frame(rgba, vis, uniforms, height, grid, count, N, high_rgba=..., low_rgba=...)

Per observer: the viewshed model's field, the radius mask (float32)(di di + dj dj) <= Rc Rc, q = rint(seen * 65536) as uint32.
The sum is an integer sum, count = (float32)sum / 65536, and the frame is the viewshed model's tint of f = count / N without a radius.
"""
from __future__ import annotations

import numpy as np

import shadow_model as shm
import viewshed_model as vsm

DEFAULTS = dict(vsm.DEFAULTS)
DEFAULT_HIGH, DEFAULT_LOW = (64, 255, 96, 160), (0, 0, 0, 0)
MAX_OBSERVERS = 65535
F32 = np.float32


def scene_observers(extra=61, seed=70):
    """The GPU tests' observers at spacing 1: the nine of tests/test_gpu_viewshed.py (corners, edges, inside, outside the grid) and
    `extra` seeded uniform ones over the grid's extent -> (9 + extra, 2) float32"""
    from test_gpu_viewshed import OBSERVERS
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array(OBSERVERS, np.float32), rng.uniform(-1.5, 1.5, (extra, 2)).astype(np.float32)])


def rc(radius, spacing, n):
    """the radius in cells, binary32: radius / (spacing step), step = 3 / (n - 1) as the vertex stage forms it"""
    step = F32(2.0 * 1.5) / (F32(n) - F32(1.0))
    with np.errstate(over="ignore", divide="ignore"):
        return F32(radius) / (F32(spacing) * step)


def in_range(n, vertex, rc_cells):
    """(n, n) bool: the vertices that count for the observer at `vertex`; the sum of squares is a 32-bit integer"""
    di = (np.arange(n, dtype=np.int64) - int(vertex[0])) ** 2
    dj = (np.arange(n, dtype=np.int64) - int(vertex[1])) ** 2
    d2 = (dj[:, None] + di[None, :]).astype(np.uint32)
    with np.errstate(over="ignore"):
        m = d2.astype(F32) <= F32(rc_cells) * F32(rc_cells)
    m[int(vertex[1]), int(vertex[0])] = True                   # (the observer's own vertex always counts)
    return m


def quantise(seen):
    return np.rint(np.ascontiguousarray(seen, F32) * F32(65536.0)).astype(np.uint32)


def sum_heights(h, vertices, exag=1.0, rc_cells=None, eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002):
    """h (n, n) float32 vertex heights, vertices [(io, jo), ...] -> (n, n) uint32, the sum of q over the observers"""
    h = np.ascontiguousarray(h, F32)
    n = h.shape[0]
    assert 1 <= len(vertices) <= MAX_OBSERVERS
    total = np.zeros((n, n), np.uint32)
    for v in vertices:
        q = quantise(vsm.field_heights(h, v, exag, eye_height, target_height, softness, bias))
        if rc_cells is not None:
            q[~in_range(n, v, rc_cells)] = 0
        total += q
    return total


def count(total):
    return np.ascontiguousarray(total, np.uint32).astype(F32) * F32(1.0 / 65536.0)


def field(uniforms, height, grid, observers, radius=None, eye_height=0.05, target_height=0.0, softness=0.02, bias=0.002, want_sum=False):
    """the count field of the renderer's surface for the uniforms' spacing and exaggeration -> (count, [(io, jo), ...])"""
    u = np.ascontiguousarray(uniforms, F32).reshape(44)
    n = max(int(grid), 2)
    spacing = max(u[36], F32(1e-8))
    vertices = [vsm.observer_vertex(o, spacing, n) for o in np.asarray(observers, F32).reshape(-1, 2)]
    total = sum_heights(shm.heights(u, height, grid), vertices, float(u[38]), None if radius is None else rc(radius, spacing, n),
                        eye_height, target_height, softness, bias)
    return (count(total), vertices, total) if want_sum else (count(total), vertices)


def fraction(cnt, observers):
    return np.ascontiguousarray(cnt, F32) / F32(observers)


def frame(rgba, vis, uniforms, height, grid, cnt, observers, high_rgba=DEFAULT_HIGH, low_rgba=DEFAULT_LOW):
    """-> (the tinted frame (H, W, 4) uint8, s (H, W) float32): the viewshed model's tint of f = count / N, over every covered pixel"""
    return vsm.frame(rgba, vis, uniforms, height, grid, fraction(cnt, observers), (0, 0), None, visible_rgba=high_rgba, hidden_rgba=low_rgba)
