#!/usr/bin/env python3
"""Cost of cast shadows (include/vf_hip.h vf_terrain_set_shadows / _read_shadow_field) at C4 (4096 x 4096, grid 4096).

The scan (k_shadow_chunk_max, k_shadow_carry, k_shadow_lit) for suns on the x axis, on the z axis, at 45 degrees and at a general
azimuth in each major axis; the shade pass (k_relight<., kShadow>) under the default and the fill camera next to the exact resolve pass of the
same frame (vf_terrain_debug_fragment_stage); and the whole shadowed frame against the unshadowed one.  Kernel times are HIP events
around `--launches` back-to-back launches after a warm-up (vf_terrain_debug_shadow_stage); the variants alternate within the process,
`--reps` rounds, and the median is reported with the spread (max - min) of the rounds.  Algorithmic bytes of a scan: 4 n^2 of heights
read once and 4 n^2 of lit written.

    python tools/exp_shadows.py [--size 4096] [--grid 4096] [--launches 20] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_shadows.py --reps 1       (the kernels by name, k_height_blocks among them)
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
SUNS = {"x axis": (1.0, 0.5, 0.0), "z axis": (0.0, 0.5, 1.0), "45 degrees": (0.7, 0.5, 0.7), "x major": (0.9, 0.5, 0.31), "z major": (0.31, 0.5, 0.9)}
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12                     # bytes / s


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
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
    t.set_shadows(True, strength=0.7, softness=0.1, bias=0.3)
    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "scan": {}, "cameras": {}}

    def with_sun(eye, sun):
        u = np.array(bench.look_at_uniforms(W, H, eye), np.float32).reshape(44)
        u[32:35] = sun
        return u

    # the scan, per sun (the shade pass of the same call is not looked at here)
    samples = {k: [] for k in SUNS}
    for r in range(a.reps):
        for k in (list(SUNS) if r % 2 == 0 else list(SUNS)[::-1]):
            t.set_uniforms(with_sun(CAMERAS["default"], SUNS[k]))
            t.render()
            samples[k].append(t.shadow_stage(a.launches)[0])
    nbytes = 8 * G * G
    for k, v in samples.items():
        med, spread = float(np.median(v)), float(max(v) - min(v))
        results["scan"][k] = {"ms": med, "spread_ms": spread, "samples_ms": v, "bytes": nbytes, "hbm_peak_share": nbytes / (med * 1e-3) / HBM_PEAK,
                              "hbm_achievable_share": nbytes / (med * 1e-3) / HBM_ACHIEVABLE}
        print(f"scan, sun {k:10s} {med:.4f} ms (spread {spread:.4f}), {nbytes / 1e6:.0f} MB, {100 * nbytes / (med * 1e-3) / HBM_ACHIEVABLE:.0f} % of achievable HBM", flush=True)
    # the shade pass and the frame, per camera
    sun = SUNS["x major"]
    for cam, eye in CAMERAS.items():
        t.set_uniforms(with_sun(eye, sun))
        samples = {"shade_pass": [], "resolve_exact": [], "frame_shadowed": [], "frame_plain": []}
        for r in range(a.reps):
            for k in (list(samples) if r % 2 == 0 else list(samples)[::-1]):
                if k == "shade_pass":
                    t.render()
                    samples[k].append(t.shadow_stage(a.launches)[1])
                elif k == "resolve_exact":
                    t.set_shade_precision(0)
                    t.render()
                    samples[k].append(t.fragment_stage(a.launches)["resolve_ms"])
                    t.set_shade_precision(1)
                else:
                    t.set_shadows(k == "frame_shadowed", strength=0.7, softness=0.1, bias=0.3)
                    for _ in range(5):
                        t.render()
                    t.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.launches):
                        t.render()
                    t.sync()
                    samples[k].append((time.perf_counter() - t0) * 1e3 / a.launches)
                    t.set_shadows(True, strength=0.7, softness=0.1, bias=0.3)
        out = {}
        for k, v in samples.items():
            out[k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
            print(f"{cam}: {k:15s} {out[k]['ms']:.4f} ms (spread {out[k]['spread_ms']:.4f})", flush=True)
        results["cameras"][cam] = out
    t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
