#!/usr/bin/env python3
"""Cost of sun exposure (include/vf_hip.h vf_terrain_set_sun_exposure / _read_sun_exposure_field) beside what a caller
pays for the same N suns with the handle's one sun and its shadow field.

Per point (grid, N), in one process, the variants alternated over `--reps` rounds, median and spread (max - min) reported:

    batched             the whole exposure field without incidence: memset, three launches per major axis and batch, the finishing
                        kernel -- HIP events around `--launches` computations after a warm-up (vf_terrain_debug_sun_exposure_stage)
    batched, incidence  the same with the incidence cosine (one slope kernel more, eight bytes more per vertex and sun)
    single scans        the yardstick: the sum over the same counted suns of one shadow scan each, HIP events as above
                        (vf_terrain_debug_shadow_stage, its scan figure)
    loop, host sum      what a caller writes today: N times set the sun + shadow_field() + a sum in numpy, by the wall clock (only at
                        points of at most `--loop-suns` suns: every turn moves grid x grid floats to the host)

The suns are N positions on a day's arc (elevation 65 sin(pi t) - 5 degrees, azimuth -90 + 180 t + 17 degrees), the first and the last
below the horizon; the weights are seeded.  `of_hbm` is the time per counted sun against the scan's algorithmic bytes, 8 n^2 (the
heights read once, one value per vertex out), at 8.0 TB/s.

    python tools/exp_sun_exposure.py [--points 512:24,512:365,1024:24,1024:365,4096:24,4096:365] [--launches 3] [--reps 5] [--batch-sizes 1,4,64]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/exp_sun_exposure.py --reps 1 --points 4096:24
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAMS = dict(softness=0.02, bias=0.002)
HBM_BYTES_PER_S = 8.0e12


def sun_vectors(N):
    k = np.float32(np.pi) / np.float32(180.0)
    t = np.linspace(0.0, 1.0, N)
    el, az = (65.0 * np.sin(np.pi * t) - 5.0).astype(np.float32) * k, (-90.0 + 180.0 * t + 17.0).astype(np.float32) * k
    return np.stack([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)], axis=1).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="512:24,512:365,1024:24,1024:365,4096:24,4096:365")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-sizes", default="", help="further arms: the batched scan without incidence at these forced batch sizes, e.g. 1,4,64")
    ap.add_argument("--loop-suns", type=int, default=24, help="the caller's loop is timed only at points of at most this many suns")
    ap.add_argument("--out", default="", help="write the JSON line to this file too")
    a = ap.parse_args(argv)
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    W = H = 64                                                # (the frame is not what is measured)
    u0 = np.array(bench.look_at_uniforms(W, H, (3.0, 2.0, 3.0)), np.float32).reshape(44)
    results = {"launches": a.launches, "reps": a.reps, "points": []}
    for point in a.points.split(","):
        G, N = (int(v) for v in point.split(":"))
        rng = np.random.default_rng(20261019)
        h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
        suns = sun_vectors(N)
        weights = rng.uniform(0.25, 1.0, N).astype(np.float32)
        counted = [s for s in suns if s[1] > 0]
        t = cabi.Terrain(W, H, G, vf.colormap_rgba8("viridis"))
        t.set_height(h)
        t.set_uniforms(u0)

        def batched(incidence, batch=0):
            t.sun_exposure_batch(batch)
            t.set_sun_exposure(suns, weights=weights, incidence=incidence, enabled=False, **PARAMS)
            return t.sun_exposure_stage(a.launches)

        def own_sun(s):
            u = u0.copy()
            u[32:35] = s
            t.set_uniforms(u)

        def single_scans():
            total = 0.0
            t.set_shadows(True, strength=1.0, **PARAMS)       # (enabled: the stage call times the frame rendered last)
            for s in counted:
                own_sun(s)
                t.render()
                total += t.shadow_stage(a.launches)[0]
            t.set_shadows(False, strength=1.0, **PARAMS)
            t.set_uniforms(u0)
            return total

        def loop_host_sum():
            t.sync()
            t0 = time.perf_counter()
            acc = np.zeros((G, G), np.float32)
            for s, w in zip(suns, weights):
                if s[1] > 0:
                    own_sun(s)
                    acc += t.shadow_field() * w
            ms = (time.perf_counter() - t0) * 1e3
            t.set_uniforms(u0)
            return ms

        variants = {"batched": lambda: batched(False), "batched, incidence": lambda: batched(True), "single scans": single_scans}
        for b in (int(v) for v in a.batch_sizes.split(",") if v):
            variants[f"batched, batch {b}"] = lambda b=b: batched(False, b)
        if N <= a.loop_suns:
            variants["loop, host sum"] = loop_host_sum
        for f in variants.values():                           # one untimed pass: allocations, first launches
            f()
        samples = {k: [] for k in variants}
        for r in range(a.reps):
            for k in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
                samples[k].append(variants[k]())
        t.sun_exposure_batch(0)
        t.set_sun_exposure(suns, weights=weights, enabled=False, **PARAMS)
        t.sun_exposure_field()
        info = t.sun_exposure_info()
        out = {"grid": G, "suns": N, "counted": info["counted"], "batch": info["batch"], "ms": {}}
        for k, v in samples.items():
            out["ms"][k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": [float(x) for x in v]}
        yard = out["ms"]["single scans"]
        per_sun_bytes = 8.0 * G * G
        for k in out["ms"]:
            if k.startswith("batched"):
                out["ms"][k]["of_single_scans"] = out["ms"][k]["ms"] / yard["ms"]
            if not k.startswith("loop"):
                out["ms"][k]["of_hbm"] = per_sun_bytes / (out["ms"][k]["ms"] * 1e-3 / info["counted"]) / HBM_BYTES_PER_S
        results["points"].append(out)
        print(f"grid {G} N {N} batch {out['batch']}: " + "; ".join(f"{k} {v['ms']:.3f} ms (spread {v['spread_ms']:.3f})" for k, v in out["ms"].items()), flush=True)
        t.close()
    line = json.dumps(results)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
