"""What the GPU overlay tests (test_gpu_overlays / _polygons / _occlusion) share: the grid, the cameras, the height field, the scene
they draw, and `apply`, which makes a sequence of overlay calls on a scene and the same calls on a CPU model's layers.

    calls = [("add_points", (xyz,), dict(size_px=4.0)), ("add_polygons", (polys,), dict(fill_rgba=(0, 90, 255, 160)))]
    layers = apply(vf, scene(vf, W, H, heights()), calls, pm.Layers())
"""
import numpy as np

GRID = 1024
CAMERAS = {
    "default": ((3.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 45.0, 0.1, 100.0),
    "fill": ((0.0, 2.2, 0.01), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 60.0, 0.1, 100.0),
    "near": ((0.2, 0.6, 0.1), (1.5, 0.2, 1.2), (0.0, 1.0, 0.0), 70.0, 0.5, 100.0),   # lines and rings pass beside and behind the eye
}


def heights(seed=7, shape=(257, 311)):
    rng = np.random.default_rng(seed)
    return (rng.random(shape, dtype=np.float32) * 0.6 - 0.3).astype(np.float32)


def scene(vf, W, H, h, cam="default", precision=None):
    s = vf.Scene(W, H, grid=GRID)
    s.set_height_from_r32f(h)
    if precision is not None:
        s.set_shade_precision(precision)
    s.set_camera_look_at(*CAMERAS[cam])
    return s


def apply(vf, s, calls, layers):
    """(method, args, kwargs) calls -> made on the scene `s` and on the model `layers` (an overlay, polygon or occlusion model's
    Layers), which is returned"""
    for meth, args, kw in calls:
        getattr(s, meth)(*args, **kw)
        if meth == "add_points":
            layers.points(args[0], **kw)
        elif meth == "add_lines":
            coords, offs = vf.pack_lines(args[0])
            layers.lines([coords[offs[p]:offs[p + 1]] for p in range(len(offs) - 1)], **kw)
        else:
            coords, rings, feats = vf.pack_polygons(args[0])
            polys = [[coords[rings[r]:rings[r + 1]] for r in range(feats[f], feats[f + 1])] for f in range(len(feats) - 1)]
            layers.polygons(polys, **kw)
    return layers
