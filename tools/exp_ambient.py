#!/usr/bin/env python3
"""Cost of ambient occlusion (include/vf_hip.h vf_terrain_set_ambient / _read_sky_view_field) at C4 (4096 x 4096, grid 4096).

The field (k_ambient_dir, one launch per direction) for reach 16, 64 and 256 and one direction of each class -- on an axis, a general
x-major and z-major one, 45 degrees -- and for the default sixteen; the shade pass (k_relight<., kAmbient>) next to the cast-shadow shade
pass (k_relight<., kShadow>) of the same frame under the default and the fill camera; and the whole frame with ambient occlusion against
the plain one.  Kernel times are HIP events around `--launches` back-to-back launches after a warm-up
(vf_terrain_debug_ambient_stage / _shadow_stage); the variants alternate within the process, `--reps` rounds, and the median is
reported with the spread (max - min) of the rounds.  Slope evaluations of a field: the (vertex, predecessor) pairs the contract asks
for, n^2 R per direction; each costs the kernel one LDS read (the inverse distance) and one cross-lane read.

    python tools/exp_ambient.py [--size 4096] [--grid 4096] [--launches 10] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_ambient.py --reps 1       (the kernels by name, k_height_blocks among them)
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAMERAS = {"default": (3.0, 2.0, 3.0), "fill": (0.0, 2.2, 0.01)}
CLASSES = {"axis": (1.0, 0.0), "x major": (0.9, 0.31), "z major": (0.31, 0.9), "45 degrees": (1.0, 1.0)}
REACHES = (16.0, 64.0, 256.0)
LDS_READS_PER_S = 256 * 2.4e9 * 32                         # 256 CUs, 128 B / clk of ds_read_b32 each: dwords / s chip-wide


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=10)
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
    t.set_uniforms(np.array(bench.look_at_uniforms(W, H, CAMERAS["default"]), np.float32).reshape(44))
    t.render()
    results = {"frame": [W, H], "grid": G, "launches": a.launches, "reps": a.reps, "field": {}, "cameras": {}}

    # the field: one direction of each class and the default set, per reach
    variants = [(k, r) for r in REACHES for k in (*CLASSES, "default 16")]
    samples = {v: [] for v in variants}
    for rep in range(a.reps):
        for v in (variants if rep % 2 == 0 else variants[::-1]):
            k, r = v
            t.set_ambient_occlusion(True, reach=r, directions=16 if k == "default 16" else np.array([CLASSES[k]], np.float32))
            samples[v].append(t.ambient_stage(a.launches)[0])
    for (k, r), v in samples.items():
        dirs = [(math.cos(2 * math.pi * i / 16), math.sin(2 * math.pi * i / 16)) for i in range(16)] if k == "default 16" else [CLASSES[k]]
        evals = sum(G * G * max(1, int(r / math.hypot(1.0, min(abs(x), abs(z)) / max(abs(x), abs(z))))) for x, z in dirs)
        med, spread = float(np.median(v)), float(max(v) - min(v))
        bound = evals / LDS_READS_PER_S * 1e3
        results["field"][f"{k}, reach {r:g}"] = {"ms": med, "spread_ms": spread, "samples_ms": v, "slope_evaluations": evals, "lds_read_bound_ms": bound}
        print(f"field, {k:10s} reach {r:5g}: {med:.4f} ms (spread {spread:.4f}), {evals / 1e9:.2f} G evaluations, one LDS read each: {bound:.4f} ms at the ds_read_b32 rate", flush=True)
    # the shade pass and the frame, per camera
    P = dict(strength=0.6, reach=64.0, directions=16)
    S = dict(strength=0.7, softness=0.1, bias=0.3)
    for cam, eye in CAMERAS.items():
        u = np.array(bench.look_at_uniforms(W, H, eye), np.float32).reshape(44)
        u[32:35] = (0.9, 0.5, 0.31)
        t.set_uniforms(u)
        samples = {"ambient_shade_pass": [], "shadow_shade_pass": [], "frame_ambient": [], "frame_plain": []}
        for rep in range(a.reps):
            for k in (list(samples) if rep % 2 == 0 else list(samples)[::-1]):
                if k == "ambient_shade_pass":
                    t.set_shadows(False, **S)
                    t.set_ambient_occlusion(True, **P)
                    t.render()
                    samples[k].append(t.ambient_stage(a.launches)[1])
                elif k == "shadow_shade_pass":
                    t.set_ambient_occlusion(False, **P)
                    t.set_shadows(True, **S)
                    t.render()
                    samples[k].append(t.shadow_stage(a.launches)[1])
                    t.set_shadows(False, **S)
                else:
                    t.set_shadows(False, **S)
                    t.set_ambient_occlusion(k == "frame_ambient", **P)
                    for _ in range(5):
                        t.render()
                    t.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.launches):
                        t.render()
                    t.sync()
                    samples[k].append((time.perf_counter() - t0) * 1e3 / a.launches)
        out = {}
        for k, v in samples.items():
            out[k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
            print(f"{cam}: {k:18s} {out[k]['ms']:.4f} ms (spread {out[k]['spread_ms']:.4f})", flush=True)
        results["cameras"][cam] = out
    t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
