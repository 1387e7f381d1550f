#!/usr/bin/env python3
"""Cost of the geometry-buffer pass (include/vf_hip.h vf_terrain_gbuffer_device / _read_gbuffer / _pick) at C4
(4096 x 4096, grid 4096) under the default and the fill camera, against the fragment stage of the same frame as a launch of its own
(vf_terrain_debug_fragment_stage with the exact shade precision: k_resolve / k_resolve4).

Kernel times are HIP events around `--launches` back-to-back launches after a warm-up launch (vf_terrain_debug_gbuffer_stage); the
variants -- depth only, depth + position, all four planes, the exact and the fast resolve pass -- alternate within the process, `--reps`
rounds, and the median is reported with the spread (max - min) of the rounds.  Algorithmic bytes of a launch: 4 W H of visibility in,
4 / 12 / 12 / 4 bytes per pixel of the planes out, 16 bytes per grid vertex of records.  pick and render_gbuffer are timed end to end
on the host clock (both wait for their results).

    python tools/exp_gbuffer.py [--size 4096] [--grid 4096] [--launches 50] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_gbuffer.py --reps 1        (the kernels by name)
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
PLANE_SETS = {"depth": ("depth",), "depth+position": ("depth", "position"), "all": ("depth", "position", "normal", "primitive")}
PLANE_BYTES = {"depth": 4, "position": 12, "normal": 12, "primitive": 4}
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12                     # bytes / s


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W = H = a.size
    G = a.grid
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(20261016)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    t = cabi.Terrain(W, H, G, vf.colormap_rgba8("viridis"))
    t.set_height(h)
    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "cameras": {}}
    for cam, eye in CAMERAS.items():
        t.set_uniforms(bench.look_at_uniforms(W, H, eye))
        for _ in range(3):
            t.render()
        t.sync()
        samples = {k: [] for k in (*PLANE_SETS, "resolve_exact", "resolve_fast")}
        covered = 0
        for r in range(a.reps):
            order = list(samples) if r % 2 == 0 else list(samples)[::-1]
            for k in order:
                if k in PLANE_SETS:
                    samples[k].append(t.gbuffer_stage(PLANE_SETS[k], a.launches))
                else:
                    t.set_shade_precision(0 if k == "resolve_exact" else 1)
                    t.render()
                    ft = t.fragment_stage(a.launches)
                    samples[k].append(ft["resolve_ms"])
                    covered = ft["covered_pixels"]
        t.set_shade_precision(1)
        t.render()
        out = {"covered_pixels": int(covered), "kernels": {}}
        for k, v in samples.items():
            med, spread = float(np.median(v)), float(max(v) - min(v))
            rec = {"ms": med, "spread_ms": spread, "samples_ms": v}
            if k in PLANE_SETS:
                nbytes = W * H * (4 + sum(PLANE_BYTES[p] for p in PLANE_SETS[k])) + 16 * G * G
                rec.update(bytes=nbytes, hbm_peak_share=nbytes / (med * 1e-3) / HBM_PEAK, hbm_achievable_share=nbytes / (med * 1e-3) / HBM_ACHIEVABLE)
            out["kernels"][k] = rec
            extra = f", {rec['bytes'] / 1e6:.0f} MB, {100 * rec['hbm_achievable_share']:.0f} % of achievable HBM" if k in PLANE_SETS else ""
            print(f"{cam}: {k:15s} {med:.4f} ms (spread {spread:.4f}){extra}", flush=True)
        # end to end on the host clock: pick of n pixels against all planes with their read-back
        prng = np.random.default_rng(3)
        e2e = {}
        for n in (1, 1000, 100000):
            px = np.column_stack([prng.integers(0, W, n), prng.integers(0, H, n)]).astype(np.int32)
            t.pick(px)
            v = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                t.pick(px)
                v.append((time.perf_counter() - t0) * 1e3)
            e2e[f"pick_{n}"] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v))}
        t.read_gbuffer()
        v = []
        for _ in range(max(2, a.reps // 2)):
            t0 = time.perf_counter()
            t.read_gbuffer()
            v.append((time.perf_counter() - t0) * 1e3)
        e2e["read_gbuffer_all"] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v))}
        for k, rec in e2e.items():
            print(f"{cam}: {k:17s} {rec['ms']:.3f} ms end to end (spread {rec['spread_ms']:.3f})", flush=True)
        out["end_to_end"] = e2e
        results["cameras"][cam] = out
    t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
