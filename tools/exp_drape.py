#!/usr/bin/env python3
"""Cost of the draped image layer (include/vf_hip.h vf_terrain_set_drape) at C4 (4096 x 4096, grid 4096).

The drape shade pass (k_relight<., kDrape>, vf_terrain_debug_drape_stage) under the default and the fill camera, for opaque full-extent
images of 4096^2 and 16384^2 texels and both filters, next to the shadow shade pass (k_relight<., kShadow>: the same walk and weights
plus three field gathers, the yardstick) and the exact resolve pass of the same frame in the same session; and the whole draped frame
against the plain one.  Kernel times are HIP events around `--launches` back-to-back launches after a warm-up; the variants alternate
within the process, `--reps` rounds, and the median is reported with the spread (max - min) of the rounds.  Run it twice.

    python tools/exp_drape.py [--size 4096] [--grid 4096] [--images 4096,16384] [--launches 20] [--reps 5] [--out profiles/drape_cost_run1.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMERAS = {"default": (3.0, 2.0, 3.0), "fill": (0.0, 2.2, 0.01)}
SUN = (0.9, 0.5, 0.31)
SHADOWS = dict(strength=0.7, softness=0.1, bias=0.3)


def opaque_image(n, seed=20261018):
    """(n, n, 4) uint8: random colours, alpha 255"""
    img = np.frombuffer(np.random.default_rng(seed).bytes(n * n * 4), np.uint8).reshape(n, n, 4).copy()
    img[..., 3] = 255
    return img


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--images", default="4096,16384")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W = H = a.size
    G = a.grid
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(20261017)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    t = cabi.Terrain(W, H, G, vf.colormap_rgba8("viridis"))
    t.set_height(h)
    t.set_shadows(False, **SHADOWS)                          # (the parameters of the yardstick's field; the frames are drawn without shadows)
    sizes = [int(v) for v in a.images.split(",") if v]
    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "layout": "row-major RGBA8", "cameras": {}}
    for cam, eye in CAMERAS.items():
        u = np.array(bench.look_at_uniforms(W, H, eye), np.float32).reshape(44)
        u[32:35] = SUN
        t.set_uniforms(u)
        out = {}
        for n in sizes:
            img = opaque_image(n)
            keys = ["drape_linear", "drape_nearest", "shadow_shade", "resolve_exact", "frame_draped", "frame_plain"]
            samples = {k: [] for k in keys}
            for r in range(a.reps):
                for k in (keys if r % 2 == 0 else keys[::-1]):
                    if k.startswith("drape_"):
                        t.set_drape(img, filter=k[6:])
                        t.render()
                        samples[k].append(t.drape_stage(a.launches))
                    elif k == "shadow_shade":
                        t.render()
                        samples[k].append(t.shadow_stage(a.launches)[1])
                    elif k == "resolve_exact":
                        t.set_shade_precision(0)
                        t.render()
                        samples[k].append(t.fragment_stage(a.launches)["resolve_ms"])
                        t.set_shade_precision(1)
                    else:
                        if k == "frame_draped":
                            t.set_drape(img, filter="linear")
                        else:
                            t.clear_drape()
                        for _ in range(5):
                            t.render()
                        t.sync()
                        t0 = time.perf_counter()
                        for _ in range(a.launches):
                            t.render()
                        t.sync()
                        samples[k].append((time.perf_counter() - t0) * 1e3 / a.launches)
            t.clear_drape()
            row = {}
            for k, v in samples.items():
                row[k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
            for k in ("drape_linear", "drape_nearest"):
                row[k]["multiple_of_shadow_shade"] = row[k]["ms"] / row["shadow_shade"]["ms"]
            for k, v in row.items():
                extra = f", {v['multiple_of_shadow_shade']:.2f} x the shadow shade pass" if "multiple_of_shadow_shade" in v else ""
                print(f"{cam}, image {n}^2: {k:15s} {v['ms']:.4f} ms (spread {v['spread_ms']:.4f}){extra}", flush=True)
            out[str(n)] = row
            del img
        results["cameras"][cam] = out
    t.close()
    line = json.dumps(results, default=float)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
