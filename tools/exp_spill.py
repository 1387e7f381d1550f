#!/usr/bin/env python3
"""Cost of the spill analysis (include/vf_hip.h vf_terrain_set_spill / _read_spill_field) at C4 (4096 x 4096, grid 4096).

The field (k_spill_init, k_spill_seed, the launches of k_spill_pass with their read-backs, k_spill_out) for the two terrains of
tools/exp_flood.py: from the border (`edges`) of the smooth terrain, and from one seed at the mouth of the river-like terrain.  Each
for the group sizes of `--groups` (passes queued per read-back of their `changed` words) and, at the default group size, with the
activity flags ignored (every tile runs in every pass), with `passes`, the time per pass and tile_runs / (passes x tiles); beside them,
in the same run on the same terrain, the shadow scan for a general x-major sun and the flood's field at the median level (the smooth
terrain) or at level 0 (the river).  Then the tint pass (k_spill_tint) under the default and the fill camera next to the flood's tint
pass of the same frame.  Times are HIP events around `--launches` back-to-back computations after a warm-up
(vf_terrain_debug_spill_stage, _flood_stage, _shadow_stage; the field's figure holds the host's read-backs, which are part of it); the
variants alternate within the process, `--reps` rounds, and the median is reported with the spread (max - min) of the rounds.

    python tools/exp_spill.py [--size 4096] [--grid 4096] [--launches 3] [--reps 5] [--groups 1,4,16] [--out FILE]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from exp_flood import CAMERAS, SHADOW_SUN, river_terrain, smooth_terrain  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", default="1,4,16")
    ap.add_argument("--out", default="", help="write the JSON line to this file too")
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W = H = a.size
    G = a.grid
    tiles = ((G + 63) // 64) ** 2
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

    results = {"frame": [W, H], "grid": G, "tiles": tiles, "launches": a.launches, "reps": a.reps, "field": {}, "cameras": {}}
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
        t.set_flood(level, seeds, enabled=False)
        t.set_spill(seeds)
        t.render()
        variants = [f"group {g}" for g in groups] + ["flags ignored", "flood field", "shadow scan, x major"]
        samples = {k: [] for k in variants}
        info = {}
        for r in range(a.reps + 1):                           # (round 0: allocations and first launches, not kept)
            for k in (variants if r % 2 == 0 else variants[::-1]):
                if k.startswith("group") or k == "flags ignored":
                    t.spill_group(int(k.split()[1]) if k.startswith("group") else 0, flags=k.startswith("group"))
                    ms = t.spill_stage(a.launches)[0]
                    t.spill_field()
                    info[k] = t.spill_info()
                    t.spill_group(0)
                elif k == "flood field":
                    t.set_spill(seeds, enabled=False)
                    t.set_flood(level, seeds)
                    t.render()
                    ms = t.flood_stage(a.launches)[0]
                    info[k] = t.flood_info()
                    t.set_flood(level, seeds, enabled=False)
                    t.set_spill(seeds)
                    t.render()
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
        flood = float(np.median(samples["flood field"]))
        for k, v in samples.items():
            med, spread = float(np.median(v)), float(max(v) - min(v))
            out[k] = {"ms": med, "spread_ms": spread, "samples_ms": v}
            line = f"{name}: {k:22s} {med:.4f} ms (spread {spread:.4f})"
            if k == "flood field":
                out[k].update(passes=info[k]["passes"], flooded_vertices=info[k]["flooded_vertices"], shadow_scans=med / yard)
                line += f", {info[k]['passes']} passes, {med / yard:.1f} shadow scans"
            elif k in info:
                i = info[k]
                share = i["tile_runs"] / max(i["passes"] * tiles, 1)
                out[k].update(passes=i["passes"], ms_per_pass=med / max(i["passes"], 1), tile_runs=i["tile_runs"], tile_run_share=share,
                              reached_vertices=i["reached_vertices"], sink_vertices=i["sink_vertices"], shadow_scans=med / yard, flood_fields=med / flood)
                line += (f", {i['passes']} passes, {med / max(i['passes'], 1):.4f} ms per pass, tile runs {i['tile_runs']} ({share:.3f} of passes x tiles), "
                         f"{med / yard:.1f} shadow scans, {med / flood:.2f} flood fields, sinks {i['sink_vertices']} of {i['reached_vertices']}")
            print(line, flush=True)
        results["field"][name] = out
    # the tint pass, per camera, on the smooth terrain beside the flood's tint of the same frame
    t.spill_group(0)
    tex, _, seeds = cases["edges, smooth terrain"]
    level = results["field"]["edges, smooth terrain"]["level"]
    t.set_height(tex)
    for cam, eye in CAMERAS.items():
        t.set_uniforms(uniforms(eye))
        samples = {"spill_tint": [], "flood_tint": []}
        for r in range(a.reps + 1):
            for k in (list(samples) if r % 2 == 0 else list(samples)[::-1]):
                t.set_spill(seeds, enabled=k == "spill_tint")
                t.set_flood(level, seeds, enabled=k == "flood_tint")
                t.render()
                ms = (t.spill_stage if k == "spill_tint" else t.flood_stage)(4 * a.launches)[1]
                if r:
                    samples[k].append(ms)
        out = {}
        for k, v in samples.items():
            out[k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
            print(f"{cam}: {k:15s} {out[k]['ms']:.4f} ms (spread {out[k]['spread_ms']:.4f})", flush=True)
        out["spill_over_flood_tint"] = out["spill_tint"]["ms"] / out["flood_tint"]["ms"]
        results["cameras"][cam] = out
    t.close()
    line = json.dumps(results, default=float)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
