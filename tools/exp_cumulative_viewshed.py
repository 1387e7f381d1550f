#!/usr/bin/env python3
"""Cost of the cumulative viewshed (include/vf_hip.h vf_terrain_set_cumulative_viewshed / _read_cumulative_viewshed_field; DESIGN.md
4m) beside what a caller pays for the same N observers with the single-observer viewshed.

Per point (grid, N, radius), in one process, the variants alternated over `--reps` rounds, median and spread (max - min) reported:

    batched          the whole count field: memset, five launches per batch, the finishing kernel -- HIP events around `--launches`
                     computations after a warm-up (vf_terrain_debug_cumulative_viewshed_stage)
    single scans     the yardstick: the sum over the same N observers of one single-observer scan each, HIP events as above
                     (vf_terrain_debug_viewshed_stage); the single scan has no radius, so the radius rows share this arm's figure
    loop, device     what a caller does today without the sum: N times set_viewshed + viewshed_field_device into device memory, by
                     the wall clock around the loop (every call waits for its scan)
    loop, host sum   the same with the read-back of every field and the sum on the host (viewshed_field() and numpy)

The observers are the same N seeded positions in every arm.  The radius is a tenth of the grid's extent.

    python tools/exp_cumulative_viewshed.py [--points 512:64,512:1024,1024:64,1024:1024,4096:64] [--launches 3] [--reps 5] [--batch-sizes 1,8]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/exp_cumulative_viewshed.py --reps 1 --points 4096:64
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAMS = dict(eye_height=1.0, target_height=0.0, softness=0.1, bias=0.01)
EXTENT = 3.0                                                  # the grid spans [-1.5, 1.5] at spacing 1


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="512:64,512:1024,1024:64,1024:1024,4096:64")
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch-sizes", default="", help="further arms: the batched scan without a radius at these forced batch sizes, e.g. 1,8")
    ap.add_argument("--no-loops", action="store_true", help="leave the two caller's loops out (a kernel trace of the scans alone)")
    a = ap.parse_args(argv)
    import torch                                              # before the library: one HIP runtime per process
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    W = H = 64                                                # (the frame is not what is measured)
    u = np.array(bench.look_at_uniforms(W, H, (3.0, 2.0, 3.0)), np.float32).reshape(44)
    results = {"launches": a.launches, "reps": a.reps, "radius": EXTENT / 10.0, "points": []}
    for point in a.points.split(","):
        G, N = (int(v) for v in point.split(":"))
        rng = np.random.default_rng(20261019)
        h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
        observers = rng.uniform(-1.5, 1.5, (N, 2)).astype(np.float32)
        t = cabi.Terrain(W, H, G, vf.colormap_rgba8("viridis"))
        t.set_height(h)
        t.set_uniforms(u)
        dev = torch.empty((G, G), dtype=torch.float32, device="cuda")

        def batched(radius, batch=0):
            t.cumulative_viewshed_batch(batch)
            t.set_cumulative_viewshed(observers, enabled=False, radius=radius, **PARAMS)
            return t.cumulative_viewshed_stage(a.launches)

        def single_scans():
            total = 0.0
            for o in observers:
                t.set_viewshed(o, **PARAMS)                   # (enabled: the stage call times the frame rendered last)
                t.render()
                total += t.viewshed_stage(a.launches)[0]
            t.set_viewshed(observers[0], enabled=False, **PARAMS)
            return total

        def loop_device():
            t.sync()
            t0 = time.perf_counter()
            for o in observers:
                t.set_viewshed(o, enabled=False, **PARAMS)
                t.viewshed_field_device(dev.data_ptr())
            t.sync()
            return (time.perf_counter() - t0) * 1e3

        def loop_host_sum():
            t.sync()
            t0 = time.perf_counter()
            acc = np.zeros((G, G), np.float32)
            for o in observers:
                t.set_viewshed(o, enabled=False, **PARAMS)
                acc += t.viewshed_field()
            return (time.perf_counter() - t0) * 1e3

        variants = {"batched": lambda: batched(None), "batched, radius": lambda: batched(EXTENT / 10.0), "single scans": single_scans}
        for b in (int(v) for v in a.batch_sizes.split(",") if v):
            variants[f"batched, batch {b}"] = lambda b=b: batched(None, b)
        if not a.no_loops:
            variants.update({"loop, device": loop_device, "loop, host sum": loop_host_sum})
        for f in variants.values():                           # one untimed pass: allocations, first launches
            f()
        samples = {k: [] for k in variants}
        for r in range(a.reps):
            for k in (list(variants) if r % 2 == 0 else list(variants)[::-1]):
                samples[k].append(variants[k]())
        t.cumulative_viewshed_batch(0)
        t.set_cumulative_viewshed(observers, enabled=False, radius=None, **PARAMS)
        t.cumulative_viewshed_field()
        out = {"grid": G, "observers": N, "batch": t.cumulative_viewshed_info()["batch"], "ms": {}}
        for k, v in samples.items():
            out["ms"][k] = {"ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "samples_ms": [float(x) for x in v]}
        yard = out["ms"]["single scans"]
        for k in (k for k in out["ms"] if k.startswith("batched")):
            out["ms"][k]["of_single_scans"] = out["ms"][k]["ms"] / yard["ms"]
        results["points"].append(out)
        print(f"grid {G} N {N} batch {out['batch']}: " + "; ".join(f"{k} {v['ms']:.3f} ms (spread {v['spread_ms']:.3f})" for k, v in out["ms"].items()), flush=True)
        t.close()
        del dev
    print(json.dumps(results))


if __name__ == "__main__":
    main()
