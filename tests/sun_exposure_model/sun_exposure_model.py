"""Sun exposure's CPU model: numpy over the shadow model (tests/shadow_model).

    total = sem.sum_heights(h, suns, weights=None, spacing=1.0, exag=1.0, incidence=False, softness=0.02, bias=0.002)   # (n, n) uint32
    e = sem.exposure(total)                                                              # (n, n) float32 in [0, sum of weights]
    e = sem.field(uniforms, height, grid, suns, weights=None, incidence=False, ...)      # the renderer's own surface
    f = sem.fraction(e, sem.weight_total(suns, weights))                                 # what the tint reads
    frame, s = sem.frame(rgba, vis, uniforms, height, grid, e, wtot, high_rgba=..., low_rgba=...)
    c = sem.cosine(h, sun, spacing=1.0, exag=1.0)                                        # (n, n) float32 in [0, 1]

Per counted sun (sy > 0): the shadow model's field at strength 1, times the incidence cosine if asked, times the weight,
q = rint(v * 65536) as uint32.  The sum is an integer sum, exposure = (float32)sum / 65536, and the frame is the viewshed model's tint
of f = min(exposure / wtot, 1) without a radius.  Every operation is a binary32 one, in the order DESIGN.md 4n writes it.
"""
from __future__ import annotations

import numpy as np

import shadow_model as shm
import viewshed_model as vsm

DEFAULTS = dict(softness=0.02, bias=0.002)
DEFAULT_HIGH, DEFAULT_LOW = (255, 208, 64, 160), (0, 0, 0, 0)
MAX_SUNS = 65535
F32 = np.float32


def _arc(count=24):
    t = np.linspace(0.0, 1.0, count)
    return np.stack([shm.sun_vector(65.0 * np.sin(np.pi * tt) - 5.0, -90.0 + 180.0 * tt + 17.0) for tt in t]).astype(F32)


# The test scene's suns: 24 on an arc from sunrise to sunset (the first and the last below the horizon, twelve x-major and twelve
# z-major), then the straight-up sun, the four axes, both exact diagonals, a steep general one, a sun on the horizon and one below it.
ARC = _arc()
VECTORS = np.array([(0, 1, 0), (1, 1, 0), (0, 1, 1), (-1, 1, 0), (0, 1, -1), (1, 1, 1), (-1, 1, 1), (1, 0.5, -1), (0.3, 0, 1), (0.5, -0.2, 0.1)], F32)
SUNS = np.concatenate([ARC, VECTORS])
ARC_WEIGHTS = np.random.default_rng(24).uniform(0.25, 1.0, 24).astype(F32)
WEIGHTS = np.random.default_rng(24).uniform(0.25, 1.0, 34).astype(F32)
WEIGHTS[3] = 0.0
WEIGHTS[5] = 1.0


def _suns(suns):
    s = np.ascontiguousarray(suns, F32).reshape(-1, 3)
    assert 1 <= len(s) <= MAX_SUNS
    return s


def _weights(weights, count):
    w = np.ones(count, F32) if weights is None else np.ascontiguousarray(weights, F32).reshape(count)
    assert ((w >= 0) & (w <= 1)).all()
    return w


def counted(suns):
    """(N,) bool: the suns above the horizon"""
    return _suns(suns)[:, 1] > 0


def weight_total(suns, weights=None):
    """the binary32 sum, in list order, of the counted suns' weights"""
    s = _suns(suns)
    w = _weights(weights, len(s))
    tot = F32(0.0)
    for o in np.flatnonzero(counted(s)):
        tot = F32(tot + w[o])
    return tot


def cosine(h, sun, spacing=1.0, exag=1.0):
    """h (n, n) float32 vertex heights (row = z index, column = x index) -> c (n, n) float32: the cosine between the sun and the normal
    of the height field, central differences inside the grid and one-sided ones on its edges, clamped to [0, 1]; a NaN, and a vertex
    whose own height is not finite, give 0"""
    h = np.ascontiguousarray(h, F32)
    n = h.shape[0]
    sx, sy, sz = (F32(v) for v in np.ascontiguousarray(sun, F32).reshape(3))
    with np.errstate(all="ignore"):
        y = h * F32(exag)
        step = F32(3.0) / (F32(n) - F32(1.0))
        cell = step * F32(spacing)
        idx = np.arange(n)
        ip, im = np.minimum(idx + 1, n - 1), np.maximum(idx - 1, 0)
        span = cell * (ip - im).astype(F32)
        px = np.where(np.isfinite(y), (y[:, ip] - y[:, im]) / span[None, :], F32(np.nan))     # (a vertex without a height has no slope)
        pz = (y[ip, :] - y[im, :]) / span[:, None]
        nn = np.sqrt((F32(1.0) + px * px) + pz * pz)
        sl = np.sqrt((sx * sx + sy * sy) + sz * sz)
        c = (((sy - px * sx) - pz * sz) / nn) / sl
        return np.where(c > 0, np.minimum(c, F32(1.0)), F32(0.0)).astype(F32)


def quantise(v):
    return np.rint(np.ascontiguousarray(v, F32) * F32(65536.0)).astype(np.uint32)


def sum_heights(h, suns, weights=None, spacing=1.0, exag=1.0, incidence=False, softness=0.02, bias=0.002):
    """h (n, n) float32 vertex heights, suns (N, 3), weights (N,) or None -> (n, n) uint32, the sum of q over the counted suns"""
    h = np.ascontiguousarray(h, F32)
    s = _suns(suns)
    w = _weights(weights, len(s))
    total = np.zeros(h.shape, np.uint32)
    for o in np.flatnonzero(counted(s)):
        v = shm.field_heights(h, s[o], spacing, exag, 1.0, softness, bias)
        if incidence:
            v = v * cosine(h, s[o], spacing, exag)
        total += quantise(v * w[o])
    return total


def exposure(total):
    return np.ascontiguousarray(total, np.uint32).astype(F32) * F32(1.0 / 65536.0)


def field(uniforms, height, grid, suns, weights=None, incidence=False, softness=0.02, bias=0.002, want_sum=False):
    """the exposure field of the renderer's surface for the uniforms' spacing and exaggeration"""
    u = np.ascontiguousarray(uniforms, F32).reshape(44)
    total = sum_heights(shm.heights(u, height, grid), suns, weights, float(max(u[36], F32(1e-8))), float(u[38]), incidence, softness, bias)
    return (exposure(total), total) if want_sum else exposure(total)


def fraction(e, wtot):
    """f = wtot > 0 ? min(exposure / wtot, 1) : 0"""
    e = np.ascontiguousarray(e, F32)
    if not F32(wtot) > 0:
        return np.zeros_like(e)
    return np.minimum(e / F32(wtot), F32(1.0))


def frame(rgba, vis, uniforms, height, grid, e, wtot, high_rgba=DEFAULT_HIGH, low_rgba=DEFAULT_LOW):
    """-> (the tinted frame (H, W, 4) uint8, s (H, W) float32): the viewshed model's tint of f, over every covered pixel"""
    return vsm.frame(rgba, vis, uniforms, height, grid, fraction(e, wtot), (0, 0), None, visible_rgba=high_rgba, hidden_rgba=low_rgba)
