#!/usr/bin/env python3
"""Cost of the haze pass (include/vf_hip.h vf_terrain_set_haze) at C4's camera and grid.

For a 4096^2 frame and a 2048^2 frame with f = 2 (4096^2 samples): the haze pass alone (k_haze, vf_terrain_debug_haze_stage) with
uniform haze and with a falloff, alternated in one process with the yardstick, the viewshed tint pass with a radius on the same frame
(k_viewshed_tint, vf_terrain_debug_viewshed_stage: the same per-pixel record gathers and varyings, there before this pass was); and
the whole frame with haze against without.  Kernel times are HIP events around `--launches` launches after a warm-up, frame times
wall-clock over `--launches` back-to-back frames after a warm-up; the variants alternate, `--reps` rounds, forwards and backwards, and
the median is reported with the spread (max - min) of the rounds.  Run it twice.

    python tools/exp_haze.py [--grid 4096] [--launches 20] [--reps 5] [--out profiles/haze_cost_run1.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(4096, 1), (2048, 2)]                                # (output width = height, factor)
UNIFORM = dict(density=0.25, start=2.0)
FALLOFF = dict(density=0.25, start=2.0, falloff=0.5, base=0.0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(f"{w}x{f}" for w, f in CASES), help="output size x factor, comma separated")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    G = a.grid
    cases = [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",") if c]
    rng = np.random.default_rng(20261020)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    lut = vf.colormap_rgba8("viridis")
    results = {"grid": G, "launches": a.launches, "reps": a.reps, "camera": "C4 default (3, 2, 3)", "uniform": UNIFORM, "falloff": FALLOFF, "cases": []}
    first = None
    for size, f in cases:
        t = cabi.Terrain(size, size, G, lut, supersample=f if f > 1 else None, share_ctx=first)
        first = first or t
        t.set_height(h)
        t.set_uniforms(np.array(bench.look_at_uniforms(size, size, (3.0, 2.0, 3.0)), np.float32).reshape(44))     # C4's camera
        # the yardstick's setting is stored and enabled once (the stage call asks for that), then disabled: the stage calls time the
        # passes on the frame rendered last whatever is enabled
        tint = dict(eye_height=1.0, radius=1.0, visible_rgba=(64, 255, 96, 96), hidden_rgba=(255, 0, 0, 128))
        t.set_viewshed((0.4, 0.3), **tint)
        t.set_viewshed((0.4, 0.3), enabled=False, **tint)
        t.render()
        t.sync()

        def frame_ms(haze):
            if haze is None:
                t.clear_haze()
            else:
                t.set_haze(**haze)
            for _ in range(5):
                t.render()
            t.sync()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                t.render()
            t.sync()
            return (time.perf_counter() - t0) * 1e3 / a.launches

        def haze_ms(haze):
            t.set_haze(**haze, enabled=False)
            return t.haze_stage(a.launches)

        variants = [("tint_with_radius", lambda: t.viewshed_stage(a.launches)[1]), ("haze_uniform", lambda: haze_ms(UNIFORM)),
                    ("haze_falloff", lambda: haze_ms(FALLOFF)), ("frame_plain", lambda: frame_ms(None)), ("frame_haze_uniform", lambda: frame_ms(UNIFORM)),
                    ("frame_haze_falloff", lambda: frame_ms(FALLOFF))]
        samples = {k: [] for k, _ in variants}
        for r in range(a.reps):
            for k, fn in (variants if r % 2 == 0 else variants[::-1]):
                samples[k].append(float(fn()))
        row = {"output": [size, size], "factor": f, "raster": [size * f, size * f]}
        for k, v in samples.items():
            row[k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}
        y = row["tint_with_radius"]["ms"]
        for k in ("haze_uniform", "haze_falloff"):
            row[k + "_over_tint"] = row[k]["ms"] / y
        row["falloff_minus_uniform_ms"] = row["haze_falloff"]["ms"] - row["haze_uniform"]["ms"]
        for k in ("frame_haze_uniform", "frame_haze_falloff"):
            row[k + "_minus_plain_ms"] = row[k]["ms"] - row["frame_plain"]["ms"]
        results["cases"].append(row)
        print(f"output {size}^2, f = {f}: tint with a radius {y:.4f} ms (spread {row['tint_with_radius']['spread_ms']:.4f}); haze uniform "
              f"{row['haze_uniform']['ms']:.4f} ms = {row['haze_uniform_over_tint']:.2f} x, with a falloff {row['haze_falloff']['ms']:.4f} ms = "
              f"{row['haze_falloff_over_tint']:.2f} x; frame {row['frame_plain']['ms']:.4f} ms plain, {row['frame_haze_uniform']['ms']:.4f} uniform, "
              f"{row['frame_haze_falloff']['ms']:.4f} with a falloff", flush=True)
        if t is not first:
            t.close()
    first.close()
    line = json.dumps(results, default=float)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
