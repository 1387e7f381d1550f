#!/usr/bin/env python3
"""Cost of the flood analysis (include/vf_hip.h vf_terrain_set_flood / _read_flood_field) at C4 (4096 x 4096, grid 4096).

The field (k_flood_wet, k_flood_seed, the launches of k_flood_pass with their read-backs, k_flood_depth) for two cases: water from the
border (`edges`) at the median level of a smooth terrain, and one seed at the mouth of a river-like terrain (a meandering valley
through a plateau: the water has one long way to go).  Each for the group sizes of `--groups` (passes queued per read-back of their
`changed` words), with `passes`, the time per pass, and beside them the shadow scan for a general x-major sun, the yardstick of the
same run.  Then the tint pass (k_flood_tint) under the default and the fill camera next to the viewshed's tint pass and the exact
resolve pass of the same frame.  Times are HIP events around `--launches` back-to-back computations after a warm-up
(vf_terrain_debug_flood_stage, _viewshed_stage, _shadow_stage; the field's figure holds the host's read-backs, which are part of it);
the variants alternate within the process, `--reps` rounds, and the median is reported with the spread (max - min) of the rounds.

    python tools/exp_flood.py [--size 4096] [--grid 4096] [--launches 5] [--reps 5] [--groups 1,4,16] [--out FILE]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMERAS = {"default": (3.0, 2.0, 3.0), "fill": (0.0, 2.2, 0.01)}
SHADOW_SUN = (0.9, 0.5, 0.31)                                 # the shadow probe's general x-major sun
VIEW = dict(eye_height=1.0, target_height=0.0, softness=0.1, bias=0.01, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))


def smooth_terrain(G, seed=20261020):
    """a sum of a few long sine waves, +-0.4: lakes and hills many tiles wide"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, G, dtype=np.float32)
    X, Z = np.meshgrid(x, x)
    h = np.zeros((G, G), np.float32)
    for f in (1, 2, 3, 5, 8):
        a, p = rng.uniform(0, 6.3, 2)
        h += np.float32(rng.normal() * 0.25 / f) * np.sin(np.float32(2 * np.pi * f) * (X * np.float32(np.cos(a)) + Z * np.float32(np.sin(a))) + np.float32(p))
    return h


def river_terrain(G):
    """a plateau at +1 with one meandering valley at -1, twelve bends from the edge x = 0 to the edge x = 1, G / 128 vertices wide;
    -> (texture, the vertex at its mouth).  (The renderer adds its analytic relief of +-0.5: the valley stays below 0, the plateau above.)"""
    x = np.linspace(0.0, 1.0, G, dtype=np.float32)
    X, Z = np.meshgrid(x, x)
    centre = np.float32(0.5) + np.float32(0.4) * np.sin(np.float32(2 * np.pi * 12) * X)
    # the distance to the centre line along z alone would thin the valley where it is steep: widen by the slope
    slope = np.float32(0.4 * 2 * np.pi * 12) * np.abs(np.cos(np.float32(2 * np.pi * 12) * X))
    half = np.float32(1.0 / 256.0) * np.sqrt(np.float32(1.0) + slope * slope)
    h = np.where(np.abs(Z - centre) <= half, np.float32(-1.0), np.float32(1.0)).astype(np.float32)
    return h, (0, int(round(0.5 * (G - 1))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", default="1,4,16")
    ap.add_argument("--out", default="", help="write the JSON line to this file too")
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W = H = a.size
    G = a.grid
    groups = [int(v) for v in a.groups.split(",") if v]
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def uniforms(eye):
        u = np.array(bench.look_at_uniforms(W, H, eye), np.float32).reshape(44)
        u[32:35] = SHADOW_SUN
        return u

    def vertex_xz(v):
        step = 3.0 / (G - 1)
        return (-1.5 + v[0] * step, -1.5 + v[1] * step)

    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "field": {}, "cameras": {}}
    t = cabi.Terrain(W, H, G, vf.colormap_rgba8("viridis"))
    t.set_uniforms(uniforms(CAMERAS["default"]))
    smooth = smooth_terrain(G)
    river, mouth = river_terrain(G)
    cases = {"edges, smooth terrain": (smooth, None, "edges"), "one seed, river": (river, 0.0, [vertex_xz(mouth)])}
    for name, (tex, level, seeds) in cases.items():
        t.set_height(tex)
        if level is None:                                     # the median of the surface the renderer draws: by bisection on the wet-able count
            lo, hi = -2.0, 2.0
            for _ in range(20):
                level = 0.5 * (lo + hi)
                t.set_flood(level, None, enabled=False)
                t.flood_field()
                lo, hi = (level, hi) if t.flood_info()["wettable_vertices"] < G * G // 2 else (lo, level)
        t.set_shadows(False, strength=0.7, softness=0.1, bias=0.3)
        t.set_flood(level, seeds)
        t.render()
        variants = [f"group {g}" for g in groups] + ["shadow scan, x major"]
        samples = {k: [] for k in variants}
        info = {}
        for r in range(a.reps + 1):                           # (round 0: allocations and first launches, not kept)
            for k in (variants if r % 2 == 0 else variants[::-1]):
                if k.startswith("group"):
                    t.flood_group(int(k.split()[1]))
                    ms = t.flood_stage(a.launches)[0]
                    t.flood_field()
                    info[k] = t.flood_info()
                else:
                    t.set_shadows(True, strength=0.7, softness=0.1, bias=0.3)
                    t.render()
                    ms = t.shadow_stage(a.launches)[0]
                    t.set_shadows(False, strength=0.7, softness=0.1, bias=0.3)
                    t.render()
                if r:
                    samples[k].append(ms)
        out = {"level": level}
        yard = float(np.median(samples["shadow scan, x major"]))
        for k, v in samples.items():
            med, spread = float(np.median(v)), float(max(v) - min(v))
            out[k] = {"ms": med, "spread_ms": spread, "samples_ms": v}
            line = f"{name}: {k:22s} {med:.4f} ms (spread {spread:.4f})"
            if k in info:
                i = info[k]
                out[k].update(passes=i["passes"], ms_per_pass=med / max(i["passes"], 1), flooded_vertices=i["flooded_vertices"],
                              wettable_vertices=i["wettable_vertices"], shadow_scans=med / yard)
                line += f", {i['passes']} passes, {med / max(i['passes'], 1):.4f} ms per pass, {med / yard:.1f} shadow scans, flooded {i['flooded_vertices']} of {i['wettable_vertices']}"
            print(line, flush=True)
        results["field"][name] = out
    # the tint pass, per camera, on the smooth terrain's flood beside the viewshed tint and the exact resolve of the same frame
    t.flood_group(0)
    tex, _, seeds = cases["edges, smooth terrain"]
    t.set_height(tex)
    t.set_flood(results["field"]["edges, smooth terrain"]["level"], seeds)
    t.set_viewshed((0.0, 0.0), **VIEW)
    for cam, eye in CAMERAS.items():
        t.set_uniforms(uniforms(eye))
        samples = {"flood_tint": [], "viewshed_tint": [], "resolve_exact": []}
        for r in range(a.reps + 1):
            for k in (list(samples) if r % 2 == 0 else list(samples)[::-1]):
                t.render()
                if k == "flood_tint":
                    ms = t.flood_stage(4 * a.launches)[1]
                elif k == "viewshed_tint":
                    ms = t.viewshed_stage(4 * a.launches)[1]
                else:
                    t.set_shade_precision(0)
                    t.render()
                    ms = t.fragment_stage(4 * a.launches)["resolve_ms"]
                    t.set_shade_precision(1)
                if r:
                    samples[k].append(ms)
        out = {}
        for k, v in samples.items():
            out[k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
            print(f"{cam}: {k:15s} {out[k]['ms']:.4f} ms (spread {out[k]['spread_ms']:.4f})", flush=True)
        out["flood_over_viewshed_tint"] = out["flood_tint"]["ms"] / out["viewshed_tint"]["ms"]
        results["cameras"][cam] = out
    t.close()
    line = json.dumps(results, default=float)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
