#!/usr/bin/env python3
"""Cost of the viewshed analysis (include/vf_hip.h vf_terrain_set_viewshed / _read_viewshed_field) at C4 (4096 x 4096,
grid 4096).

The scan (k_viewshed_chunk_max, k_viewshed_carry, k_viewshed_seen) for an observer at the centre, in a corner and on an edge, beside
the shadow scan for a general x-major sun as a yardstick of the same run; the tint pass (k_viewshed_tint) under the default and the
fill camera next to the exact resolve pass of the same frame (vf_terrain_debug_fragment_stage); and the whole tinted frame against the
untinted one.  Kernel times are HIP events around `--launches` back-to-back launches after a warm-up (vf_terrain_debug_viewshed_stage,
_shadow_stage); the variants alternate within the process, `--reps` rounds, and the median is reported with the spread (max - min) of
the rounds.  Algorithmic bytes of a scan: 4 n^2 of heights read once and 4 n^2 of seen written.  The heights are uploaded again in
every round, so a kernel trace of the probe holds k_height_blocks (the other yardstick: the same volume in the same layout) `--reps` times.

    python tools/exp_viewshed.py [--size 4096] [--grid 4096] [--launches 20] [--reps 5]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/exp_viewshed.py --reps 1       (the kernels by name, k_height_blocks among them)
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
OBSERVERS = {"centre": (0.0, 0.0), "corner": (-1.5, -1.5), "edge": (0.0, -1.5)}
SHADOW_SUN = (0.9, 0.5, 0.31)                                 # the shadow probe's general x-major sun
PARAMS = dict(eye_height=1.0, target_height=0.0, softness=0.1, bias=0.01)
TINT = dict(visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))
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
    rng = np.random.default_rng(20261019)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    t = cabi.Terrain(W, H, G, vf.colormap_rgba8("viridis"))
    t.set_height(h)
    t.set_shadows(False, strength=0.7, softness=0.1, bias=0.3)
    t.set_viewshed(OBSERVERS["centre"], **PARAMS, **TINT)
    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "scan": {}, "cameras": {}}

    def uniforms(eye):
        u = np.array(bench.look_at_uniforms(W, H, eye), np.float32).reshape(44)
        u[32:35] = SHADOW_SUN
        return u

    # the scan, per observer, and the shadow scan beside it (the passes of the same calls are not looked at here)
    t.set_uniforms(uniforms(CAMERAS["default"]))
    variants = list(OBSERVERS) + ["shadow scan, x major"]
    samples = {k: [] for k in variants}
    for r in range(a.reps):
        t.set_height(h)                                       # (k_height_blocks once more, for a kernel trace)
        for k in (variants if r % 2 == 0 else variants[::-1]):
            if k in OBSERVERS:
                t.set_viewshed(OBSERVERS[k], **PARAMS, **TINT)
                t.render()
                samples[k].append(t.viewshed_stage(a.launches)[0])
            else:
                t.set_shadows(True, strength=0.7, softness=0.1, bias=0.3)
                t.render()
                samples[k].append(t.shadow_stage(a.launches)[0])
                t.set_shadows(False, strength=0.7, softness=0.1, bias=0.3)
    nbytes = 8 * G * G
    for k, v in samples.items():
        med, spread = float(np.median(v)), float(max(v) - min(v))
        results["scan"][k] = {"ms": med, "spread_ms": spread, "samples_ms": v, "bytes": nbytes, "hbm_peak_share": nbytes / (med * 1e-3) / HBM_PEAK,
                              "hbm_achievable_share": nbytes / (med * 1e-3) / HBM_ACHIEVABLE}
        print(f"scan, {k:22s} {med:.4f} ms (spread {spread:.4f}), {nbytes / 1e6:.0f} MB, {100 * nbytes / (med * 1e-3) / HBM_ACHIEVABLE:.0f} % of achievable HBM", flush=True)
    # the tint pass and the frame, per camera
    t.set_viewshed(OBSERVERS["centre"], **PARAMS, **TINT)
    for cam, eye in CAMERAS.items():
        t.set_uniforms(uniforms(eye))
        samples = {"tint_pass": [], "resolve_exact": [], "frame_tinted": [], "frame_plain": []}
        for r in range(a.reps):
            for k in (list(samples) if r % 2 == 0 else list(samples)[::-1]):
                if k == "tint_pass":
                    t.render()
                    samples[k].append(t.viewshed_stage(a.launches)[1])
                elif k == "resolve_exact":
                    t.set_shade_precision(0)
                    t.render()
                    samples[k].append(t.fragment_stage(a.launches)["resolve_ms"])
                    t.set_shade_precision(1)
                else:
                    t.set_viewshed(OBSERVERS["centre"], enabled=k == "frame_tinted", **PARAMS, **TINT)
                    for _ in range(5):
                        t.render()
                    t.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.launches):
                        t.render()
                    t.sync()
                    samples[k].append((time.perf_counter() - t0) * 1e3 / a.launches)
                    t.set_viewshed(OBSERVERS["centre"], **PARAMS, **TINT)
        out = {}
        for k, v in samples.items():
            out[k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
            print(f"{cam}: {k:15s} {out[k]['ms']:.4f} ms (spread {out[k]['spread_ms']:.4f})", flush=True)
        results["cameras"][cam] = out
    t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
