#!/usr/bin/env python3
"""Cost of hazed overlay layers per frame (include/vf_hip.h vf_terrain_set_layer_haze) at 1920 x 1080 on a grid-1024
handle with haze enabled and a falloff (so the opacity takes its three-exponential path): 1 M draped 4-px points, and 1 M draped 2-px
segments (1 M two-vertex paths, butt caps), over the default camera's orbit.

One handle per workload; the layer's flags are switched between the variants -- plain, hazed, occluding, hazed and occluding -- so the
same records, terrain and haze pass are drawn every time and the differences are the overlay pass's: k_ov_haze_setup and
k_ov_composite_haze against k_ov_composite, and in the same process the yardstick, k_ov_composite_occlude against k_ov_composite
(the handle's haze stores the visibility in every variant, so the yardstick here holds the composite's share of what 4d measured).
A variant's time is wall-clock over `--poses` back-to-back frames after a warm-up; the variants alternate, `--reps` rounds, forwards
and backwards, and the median is reported with the spread (max - min) of the rounds.  Run it twice.

    python tools/exp_overlay_haze.py [--workload points|segments|both] [--poses 16] [--reps 5] [--out profiles/overlay_haze_cost_run1.json]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_overlay_haze.py --reps 2        (the kernels of both workloads)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HAZE = dict(density=0.25, start=2.0, falloff=0.5, base=0.0)
VARIANTS = [("plain", False, False), ("hazed", True, False), ("occluding", False, True), ("hazed_occluding", True, True)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["points", "segments", "both"], default="both")
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W, H, G = 1920, 1080, 1024
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(20261016)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    poses = [np.array(bench.look_at_uniforms(W, H, (3.0 * np.cos(t), 2.0, 3.0 * np.sin(t))), np.float32).reshape(44)
             for t in np.linspace(0, 2 * np.pi, a.poses, endpoint=False)]
    lut = vf.colormap_rgba8("viridis")
    n = a.n
    results = {"frame": [W, H], "grid": G, "poses": a.poses, "reps": a.reps, "primitives": n, "haze": HAZE}
    for name in (["points", "segments"] if a.workload == "both" else [a.workload]):
        xz = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
        t = cabi.Terrain(W, H, G, lut)
        t.set_height(h)
        t.set_haze(**HAZE)
        if name == "points":
            xyz = np.column_stack([xz[:, 0], np.full(n, 0.02, np.float32), xz[:, 1]]).astype(np.float32)
            layer = t.add_points(xyz, size_px=4.0, rgba=(255, 80, 40, 200), shape=0, drape=True)
        else:
            d = np.random.default_rng(7).normal(0, 0.01, (n, 2)).astype(np.float32)
            coords = np.empty((2 * n, 3), np.float32)
            coords[0::2, 0], coords[0::2, 2] = xz[:, 0], xz[:, 1]
            coords[1::2, 0], coords[1::2, 2] = xz[:, 0] + d[:, 0], xz[:, 1] + d[:, 1]
            coords[:, 1] = 0.02
            layer = t.add_lines(coords, np.arange(0, 2 * n + 1, 2, dtype=np.uint32), width_px=2.0, rgba=(40, 200, 255, 220), cap=0, drape=True)

        def orbit():
            for u in poses:
                t.set_uniforms(u)
                t.render()
            t.sync()

        def frame_ms(haze, occlude):
            t.set_layer_haze(layer, haze)
            t.set_layer_occlusion(layer, occlude)
            orbit()                                               # warm-up (plans, pair list sized)
            t0 = time.perf_counter()
            orbit()
            return (time.perf_counter() - t0) * 1e3 / len(poses)

        samples = {k: [] for k, _, _ in VARIANTS}
        for r in range(a.reps):
            for k, hz, oc in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
                samples[k].append(float(frame_ms(hz, oc)))
        row = {k: {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v} for k, v in samples.items()}
        row["haze_ms_per_frame"] = row["hazed"]["ms"] - row["plain"]["ms"]
        row["occlusion_ms_per_frame"] = row["occluding"]["ms"] - row["plain"]["ms"]
        row["haze_on_occluding_ms_per_frame"] = row["hazed_occluding"]["ms"] - row["occluding"]["ms"]
        results[name] = row
        print(f"{name}: frame {row['plain']['ms']:.3f} ms plain, {row['hazed']['ms']:.3f} hazed (+{row['haze_ms_per_frame']:.3f}), "
              f"{row['occluding']['ms']:.3f} occluding (+{row['occlusion_ms_per_frame']:.3f}), {row['hazed_occluding']['ms']:.3f} both "
              f"(+{row['haze_on_occluding_ms_per_frame']:.3f} on occluding); spreads "
              + ", ".join(f"{row[k]['spread_ms']:.3f}" for k, _, _ in VARIANTS), flush=True)
        t.close()
    line = json.dumps(results, default=float)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
