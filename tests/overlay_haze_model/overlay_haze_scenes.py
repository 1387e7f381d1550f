"""What tests/test_gpu_overlay_haze.py draws and tests/test_overlay_haze_model.py holds to the conditions that keep the GPU comparison
from being vacuous ("What was verified"): the frame sizes, the haze settings per camera and the hazed layers, as
(method, args, kwargs) calls for overlay_scenes.apply.  The grid, the heights and the cameras are overlay_scenes' (tests/test_gpu_haze.py's).
"""
import numpy as np

import haze_model as hzm
from overlay_scenes import CAMERAS, GRID, heights  # noqa: F401

SIZES = [(96, 64), (71, 45)]
CAMS = ["default", "fill", "near"]
ORANGE_128 = (255, 120, 40, 128)                             # haze alpha 128


def settings(cam):
    """name -> set_haze's keywords: uniform haze, the three falloffs, a cap of 0.35, haze alpha 128 (haze_model.SCENE_PARAMS: each
    camera's start sits near the first quartile of its depths)"""
    P = hzm.SCENE_PARAMS[cam]
    out = {"uniform": dict(P)}
    for f in hzm.SCENE_FALLOFFS:
        out[f"falloff {f}"] = dict(P, falloff=f, base=hzm.SCENE_BASE)
    out["capped"] = dict(P, max_opacity=0.35)
    out["alpha 128"] = dict(P, rgba=ORANGE_128)
    return out


def _spread(rng, n, y_lo, y_hi):
    """n points spread over the whole grid (|x|, |z| <= 1.45)"""
    return np.column_stack([rng.uniform(-1.45, 1.45, n), rng.uniform(y_lo, y_hi, n), rng.uniform(-1.45, 1.45, n)]).astype(np.float32)


def point_calls(seed=21, n=60):
    """circles and squares, draped and free, sizes 1, 6 and 64 px, per-feature translucent colours"""
    rng = np.random.default_rng(seed)
    calls = []
    for shape in ("circle", "square"):
        for drape in (True, False):
            for size in (1.0, 6.0, 64.0):
                m = 1 if size == 64.0 else n
                xyz = _spread(rng, m, 0.0, 0.05) if drape else _spread(rng, m, -0.1, 0.5)
                cols = rng.integers(0, 256, (m, 4), dtype=np.uint8)
                cols[:, 3] = rng.integers(90, 256, m)
                calls.append(("add_points", (xyz,), dict(size_px=size, rgba=cols, shape=shape, drape=drape, haze=True)))
    return calls


NEAR_PATH = np.array([[1.5, 0.5, -1.5], [-1.5, 0.1, 1.5], [0.2, 0.6, 0.1], [1.4, 0.1, 1.2]], np.float32)   # through the eye of `near`: clipped at its near plane
LONG_SEGMENT = np.array([[-1.5, 0.3, -1.5], [1.5, 0.3, 1.5]], np.float32)                                  # across every camera's whole depth range


def line_calls(seed=22, npaths=14):
    """caps butt, square and round, widths 1 and 5, draped and free; one long segment across the depth range and one path through the
    near plane of the `near` camera"""
    rng = np.random.default_rng(seed)
    calls = []
    k = 0
    for cap in ("butt", "square", "round"):
        for width in (1.0, 5.0):
            drape = k % 2 == 0
            paths = []
            for _ in range(npaths):
                m = int(rng.integers(2, 6))
                start = rng.uniform(-1.4, 1.4, 3) * [1, 0.05, 1] + [0, 0.02 if drape else 0.2, 0]
                paths.append((start + np.cumsum(rng.normal(0, 0.25, (m, 3)) * [1, 0.04, 1], axis=0)).astype(np.float32))
            if k == 1:
                paths += [LONG_SEGMENT, NEAR_PATH]
            calls.append(("add_lines", (paths,), dict(width_px=width, rgba=(255 - 40 * k, 30 * k, 120, 255 if k % 3 else 170), cap=cap,
                                                      drape=drape, haze=True)))
            k += 1
    return calls


def near_points():
    """free points close in front of the eye of `fill` (view depth about 1.3 against start 2.5) and of `near` (about 0.8 along its
    axis, between its near plane at 0.5 and start 1.1): nearer than `start`, so their haze opacity is 0"""
    return {"fill": np.array([[0.0, 0.9, 0.0], [0.2, 0.8, 0.1]], np.float32),
            "near": np.array([[0.794, 0.417, 0.603], [0.85, 0.40, 0.62]], np.float32)}


def band_points(seed=23, n=40):
    """draped 24-px squares on the strip of the grid that the `default` camera sees at depths 4.5 to 5.2 (x + z from 1.9 to 2.4): just
    behind its `start`, where the opacity is still under the cap of 0.35 -- the points spread over the whole grid are mostly beyond it"""
    rng = np.random.default_rng(seed)
    s, t = rng.uniform(1.9, 2.4, n), rng.uniform(-0.45, 0.45, n)
    xyz = np.column_stack([(s + t) / 2, np.full(n, 0.02), (s - t) / 2]).astype(np.float32)
    return ("add_points", (xyz,), dict(size_px=24.0, rgba=(30, 60, 200, 140), shape="square", drape=True, haze=True))


def layer_calls(cam):
    """every hazed point and line layer of a frame test, in layer order"""
    calls = point_calls() + line_calls()
    if cam == "default":
        calls.append(band_points())
    if cam in near_points():
        calls.append(("add_points", (near_points()[cam],), dict(size_px=6.0, rgba=(255, 255, 0, 255), drape=False, haze=True)))
    return calls
