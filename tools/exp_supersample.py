#!/usr/bin/env python3
"""Cost of supersampled terrain frames (include/vf_hip.h vf_terrain_create_supersampled) at C4's camera and grid.

For output 4096^2 with f = 2 and output 2048^2 with f = 2, 3, 4: the frame time of the supersampled handle against the f = 1 frame of
the same output size and against the f = 1 frame of the sample size; and the resolve alone (k_ss_resolve<f>,
vf_terrain_debug_resolve_stage) in ms and in GB/s of its algorithmic bytes, (4 f^2 + 4) W H.  The yardstick of the same run: the
fragment-stage diagnostic of the f = 1 handles (k_resolve4, vf_terrain_debug_fragment_stage: 4 bytes of visibility in, 4 bytes of colour
out per pixel plus its record gathers), in GB/s of 8 W H.  Frame times are wall-clock over `--launches` back-to-back frames after a
warm-up, kernel times HIP events around `--launches` launches after a warm-up; the variants alternate within the process, `--reps`
rounds, forwards and backwards, and the median is reported with the spread (max - min) of the rounds.  Run it twice.

    python tools/exp_supersample.py [--grid 4096] [--launches 20] [--reps 5] [--out profiles/supersample_cost_run1.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(4096, 2), (2048, 2), (2048, 3), (2048, 4)]          # (output width = height, factor)


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
    rng = np.random.default_rng(20261017)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    lut = vf.colormap_rgba8("viridis")
    first = None

    def handle(size, f):
        nonlocal first
        t = cabi.Terrain(size, size, G, lut, supersample=f if f > 1 else None, share_ctx=first)
        first = first or t
        t.set_height(h)
        t.set_uniforms(np.array(bench.look_at_uniforms(size, size, (3.0, 2.0, 3.0)), np.float32).reshape(44))     # C4's camera (the aspect is 1 at every size)
        return t

    # the handles: every supersampled case, and one f = 1 handle per output size and per sample size
    plain_sizes = sorted({w for w, _ in cases} | {w * f for w, f in cases})
    plain = {w: handle(w, 1) for w in plain_sizes}
    ss = {(w, f): handle(w, f) for w, f in cases}
    keys = [("frame", ("plain", w)) for w in plain_sizes] + [("frame", ("ss",) + c) for c in cases] + \
           [("resolve", c) for c in cases] + [("fragment", w) for w in plain_sizes]
    samples = {k: [] for k in keys}

    def frame_ms(t):
        for _ in range(5):
            t.render()
        t.sync()
        t0 = time.perf_counter()
        for _ in range(a.launches):
            t.render()
        t.sync()
        return (time.perf_counter() - t0) * 1e3 / a.launches

    for r in range(a.reps):
        for k in (keys if r % 2 == 0 else keys[::-1]):
            kind, what = k
            if kind == "frame":
                samples[k].append(frame_ms(plain[what[1]] if what[0] == "plain" else ss[what[1:]]))
            elif kind == "resolve":
                t = ss[what]
                t.render()
                samples[k].append(t.resolve_stage(a.launches))
            else:
                t = plain[what]
                t.render()
                samples[k].append(t.fragment_stage(a.launches)["resolve_ms"])

    def stat(k):
        v = samples[k]
        return {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": v}

    results = {"grid": G, "launches": a.launches, "reps": a.reps, "camera": "C4 default (3, 2, 3)", "plain_frames": {}, "fragment_stage": {}, "cases": []}
    for w in plain_sizes:
        results["plain_frames"][str(w)] = stat(("frame", ("plain", w)))
        fr = stat(("fragment", w))
        fr["algorithmic_bytes"] = 8 * w * w
        fr["GB_per_s"] = fr["algorithmic_bytes"] / (fr["ms"] * 1e-3) / 1e9
        results["fragment_stage"][str(w)] = fr
        print(f"f = 1, {w}^2: frame {results['plain_frames'][str(w)]['ms']:.4f} ms; fragment stage {fr['ms']:.4f} ms = {fr['GB_per_s']:.0f} GB/s of 8 W H", flush=True)
    best = max(v["GB_per_s"] for v in results["fragment_stage"].values())
    results["yardstick_GB_per_s"] = best
    for w, f in cases:
        fr, rs = stat(("frame", ("ss", w, f))), stat(("resolve", (w, f)))
        same, big = results["plain_frames"][str(w)]["ms"], results["plain_frames"][str(w * f)]["ms"]
        nbytes = (4 * f * f + 4) * w * w
        row = {"output": [w, w], "factor": f, "samples": [w * f, w * f], "frame": fr, "frame_over_plain_same_output": fr["ms"] / same,
               "frame_over_plain_sample_size": fr["ms"] / big, "frame_minus_plain_sample_size_ms": fr["ms"] - big, "resolve": rs,
               "resolve_algorithmic_bytes": nbytes, "resolve_GB_per_s": nbytes / (rs["ms"] * 1e-3) / 1e9}
        row["resolve_share_of_yardstick"] = row["resolve_GB_per_s"] / best
        results["cases"].append(row)
        print(f"output {w}^2, f = {f}: frame {fr['ms']:.4f} ms (spread {fr['spread_ms']:.4f}) = {row['frame_over_plain_same_output']:.2f} x the f = 1 frame of {w}^2, "
              f"{row['frame_over_plain_sample_size']:.3f} x the f = 1 frame of {w * f}^2; resolve {rs['ms']:.4f} ms (spread {rs['spread_ms']:.4f}) = "
              f"{row['resolve_GB_per_s']:.0f} GB/s of (4 f^2 + 4) W H, {row['resolve_share_of_yardstick']:.2f} of the fragment stage's best", flush=True)
    for t in list(ss.values()) + [p for p in plain.values() if p is not first]:
        t.close()
    first.close()
    line = json.dumps(results, default=float)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
