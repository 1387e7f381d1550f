#!/usr/bin/env python3
"""Cost of overlay occlusion per frame (include/vf_hip.h vf_terrain_set_layer_occlusion) at 1920 x 1080 on a grid-1024
Scene-like handle: 1 M draped 4-px points, and 1 M draped 2-px segments (1 M two-vertex paths, butt caps), over the default camera's
orbit -- the same layer on two handles of the same terrain, one occluding and one not.

Both handles draw the same batch of poses into device buffers (vf_terrain_render_batch on the library's stream), bracketed by device
events; they alternate A B A B within the process, and the difference of the medians is what occlusion adds per frame (the terrain
pass with the visibility store, the composite's per-pixel terrain depth and per-primitive test).

    python tools/exp_occlusion.py [--workload points|segments|both] [--poses 16] [--reps 7]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_occlusion.py --reps 2        (the kernels of both workloads)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["points", "segments", "both"], default="both")
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args(argv)
    import torch
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W, H, G = 1920, 1080, 1024
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(20261016)
    h = (rng.random((G, G), dtype=np.float32) * np.float32(0.5) - np.float32(0.25)).astype(np.float32)
    poses = np.stack([bench.look_at_uniforms(W, H, (3.0 * np.cos(t), 2.0, 3.0 * np.sin(t))) for t in np.linspace(0, 2 * np.pi, a.poses, endpoint=False)])
    lut = vf.colormap_rgba8("viridis")
    n = 1_000_000
    results = {"frame": [W, H], "grid": G, "poses": a.poses, "reps": a.reps, "goal_ms": 0.5}
    first = None
    for name in (["points", "segments"] if a.workload == "both" else [a.workload]):
        xz = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
        handles = {}
        for key in ("occluding", "plain"):
            t = cabi.Terrain(W, H, G, lut, share_ctx=first)
            first = first or t
            t.set_height(h)
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
            if key == "occluding":
                t.set_layer_occlusion(layer, True)
            handles[key] = t
        stream = torch.cuda.ExternalStream(first.stream_handle())   # the library's own stream: the events go where the frames are drawn
        outs = [torch.empty(H * W * 4, dtype=torch.uint8, device="cuda") for _ in range(a.poses)]
        ptrs = [o.data_ptr() for o in outs]
        torch.cuda.synchronize()
        ms = {"occluding": [], "plain": []}
        for handle in handles.values():                         # warm-up (plans, pair list sized)
            handle.render_batch(poses, ptrs, stream.cuda_stream)
        torch.cuda.synchronize()
        for r in range(a.reps):
            for key in (("occluding", "plain") if r % 2 == 0 else ("plain", "occluding")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                handles[key].render_batch(poses, ptrs, stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1) / a.poses)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        results[name] = {"frame_ms_occluding": med["occluding"], "frame_ms_plain": med["plain"],
                         "occlusion_ms_per_frame": med["occluding"] - med["plain"], "samples_ms": ms}
        print(f"{name}: frame {med['plain']:.3f} ms with a plain layer, {med['occluding']:.3f} ms occluding: occlusion costs "
              f"{med['occluding'] - med['plain']:.3f} ms per frame (goal <= 0.5 ms)", flush=True)
        for key, t in handles.items():
            if t is not first:
                t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
