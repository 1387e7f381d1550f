#!/usr/bin/env python3
"""Cost of polygon overlays per frame (include/vf_hip.h, vf_terrain_add_polygons) at 1920 x 1080 on a grid-1024
Scene-like handle, over the default camera's orbit:
  fill       10 000 draped polygons, each a 64-vertex exterior with one 32-vertex hole (~1 M ring edges), fill only
  outlined   the same with a 1-px outline
  ring       one 200 000-vertex ring covering most of the screen, fill only

Two handles of the same terrain -- one with the workload's layer, one without -- draw the same batch of poses into device buffers
(vf_terrain_render_batch on the library's stream), bracketed by device events; the two alternate A B A B within the process, and the
difference of the medians is the layer's cost per frame.

    python tools/exp_polygons.py [--workload fill|outlined|ring|all] [--poses 8] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_polygons.py --reps 2        (the kernels of the workloads)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ring(c, r, n, phase, reverse=False):
    a = phase + np.linspace(0, 2 * np.pi, n, endpoint=False)
    p = np.column_stack([c[0] + r * np.cos(a), np.full(n, 0.02), c[1] + r * np.sin(a)]).astype(np.float32)
    return p[::-1] if reverse else p


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["fill", "outlined", "ring", "all"], default="all")
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
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
    results = {"frame": [W, H], "grid": G, "poses": a.poses, "reps": a.reps, "goal_ms": 3.0}
    plain = cabi.Terrain(W, H, G, lut)
    plain.set_height(h)
    stream = torch.cuda.ExternalStream(plain.stream_handle())   # the library's own stream: the events go where the frames are drawn
    outs = [torch.empty(H * W * 4, dtype=torch.uint8, device="cuda") for _ in range(a.poses)]
    ptrs = [o.data_ptr() for o in outs]
    torch.cuda.synchronize()
    centres = rng.uniform(-1.45, 1.45, (10_000, 2))
    radii = rng.uniform(0.01, 0.03, 10_000)
    polys = [[ring(c, r, 64, rng.uniform(0, 1)), ring(c, 0.5 * r, 32, rng.uniform(0, 1), reverse=True)] for c, r in zip(centres, radii)]
    for name in (["fill", "outlined", "ring"] if a.workload == "all" else [a.workload]):
        t = cabi.Terrain(W, H, G, lut, share_ctx=plain)
        t.set_height(h)
        if name == "ring":
            n = 200_000
            ang = np.linspace(0, 2 * np.pi, n, endpoint=False)
            r = 1.3 + 0.1 * np.sin(41 * ang)
            big = np.column_stack([r * np.cos(ang), np.full(n, 0.02), r * np.sin(ang)]).astype(np.float32)
            coords, ro, fo = vf.pack_polygons([big])
            t.add_polygons(coords, ro, fo, fill_rgba=(60, 60, 255, 150), drape=True)
        else:
            coords, ro, fo = vf.pack_polygons(polys)
            t.add_polygons(coords, ro, fo, fill_rgba=(255, 80, 40, 160), line_rgba=(20, 20, 20, 255) if name == "outlined" else None,
                           line_width_px=1.0, drape=True)
        ms = {"with": [], "without": []}
        for handle in (t, plain):                               # warm-up (plans, pair list and masks sized)
            handle.render_batch(poses, ptrs, stream.cuda_stream)
        torch.cuda.synchronize()
        for rep in range(a.reps):
            for key, handle in (("with", t), ("without", plain)) if rep % 2 == 0 else (("without", plain), ("with", t)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                handle.render_batch(poses, ptrs, stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1) / a.poses)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        results[name] = {"frame_ms_with": med["with"], "frame_ms_without": med["without"],
                         "polygon_ms_per_frame": med["with"] - med["without"], "samples_ms": ms}
        print(f"{name}: frame {med['without']:.3f} ms without, {med['with']:.3f} ms with polygons: the layer costs "
              f"{med['with'] - med['without']:.3f} ms per frame (goal for the 10k fill <= 3 ms)", flush=True)
        t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
