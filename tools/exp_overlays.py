#!/usr/bin/env python3
"""Cost of the overlay pass per frame (include/vf_hip.h, overlays; vulkan_forge_amd/csrc/vf_overlay.h) at 1920 x 1080 on a grid-1024
Scene-like handle: 1 M 4-px points, and 1 M 2-px segments (1 M two-vertex paths, butt caps), over the default camera's orbit.

Two handles of the same terrain -- one with the workload's layer, one without -- draw the same batch of poses into device buffers
(vf_terrain_render_batch on the library's stream), bracketed by device events; the two alternate A B A B within the process, and the
difference of the medians is the pass's cost per frame.

    python tools/exp_overlays.py [--workload points|segments|both] [--poses 16] [--reps 7]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_overlays.py --reps 2        (the kernels of both workloads)
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
    results = {"frame": [W, H], "grid": G, "poses": a.poses, "reps": a.reps, "goal_ms": 2.0}
    plain = cabi.Terrain(W, H, G, lut)
    plain.set_height(h)
    stream = torch.cuda.ExternalStream(plain.stream_handle())   # the library's own stream: the events go where the frames are drawn
    outs = [torch.empty(H * W * 4, dtype=torch.uint8, device="cuda") for _ in range(a.poses)]
    ptrs = [o.data_ptr() for o in outs]
    torch.cuda.synchronize()
    for name in (["points", "segments"] if a.workload == "both" else [a.workload]):
        t = cabi.Terrain(W, H, G, lut, share_ctx=plain)
        t.set_height(h)
        xz = rng.uniform(-1.5, 1.5, (n, 2)).astype(np.float32)
        if name == "points":
            xyz = np.column_stack([xz[:, 0], np.full(n, 0.02, np.float32), xz[:, 1]]).astype(np.float32)
            t.add_points(xyz, size_px=4.0, rgba=(255, 80, 40, 200), shape=0, drape=True)
        else:
            d = rng.normal(0, 0.01, (n, 2)).astype(np.float32)
            coords = np.empty((2 * n, 3), np.float32)
            coords[0::2, 0], coords[0::2, 2] = xz[:, 0], xz[:, 1]
            coords[1::2, 0], coords[1::2, 2] = xz[:, 0] + d[:, 0], xz[:, 1] + d[:, 1]
            coords[:, 1] = 0.02
            t.add_lines(coords, np.arange(0, 2 * n + 1, 2, dtype=np.uint32), width_px=2.0, rgba=(40, 200, 255, 220), cap=0, drape=True)
        ms = {"with": [], "without": []}
        for handle in (t, plain):                               # warm-up (plans, pair list sized)
            handle.render_batch(poses, ptrs, stream.cuda_stream)
        torch.cuda.synchronize()
        for r in range(a.reps):
            for key, handle in (("with", t), ("without", plain)) if r % 2 == 0 else (("without", plain), ("with", t)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                handle.render_batch(poses, ptrs, stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1) / a.poses)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        results[name] = {"frame_ms_with": med["with"], "frame_ms_without": med["without"],
                         "overlay_ms_per_frame": med["with"] - med["without"], "samples_ms": ms}
        print(f"{name}: frame {med['without']:.3f} ms without, {med['with']:.3f} ms with overlays: the pass costs "
              f"{med['with'] - med['without']:.3f} ms per frame (goal <= 2 ms)", flush=True)
        t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
