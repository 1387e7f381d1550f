#!/usr/bin/env python3
"""Cost of contour layers (include/vf_hip.h vf_terrain_add_contours) at 1920 x 1080 on grids 1024 and 4096, 20 and 200
levels spread over the surface's height bounds, on a smooth synthetic terrain (a sum of ridges and hills; white noise would cross
every level in every triangle).  VF_JOIN_NONE, so that a contour layer and the same segments added through vf_terrain_add_lines
(two-vertex paths, butt caps) are the same records but for their feature numbers: one feature against one per segment (so the
frames differ where segments overlap: add_lines blends each segment, a contour layer the maximum of their coverage).

(a) add time: the wall time of vf_terrain_add_contours (it returns after the extraction) against the host route, the only one a caller
    has without it: form the rendered surface on the CPU, extract the segments with the CPU model (tests/contour_model, its
    bracketed search) and hand them to vf_terrain_add_lines -- each part timed.
(b) frame time: a handle with the contour layer, a handle with the same segments through add_lines, and a handle without overlays draw
    the same batch of poses into device buffers (vf_terrain_render_batch on the library's stream, device events), alternated in one
    process; medians of --reps runs, and the spread of each.

    python tools/exp_contours.py [--grids 1024 4096] [--levels 20 200] [--poses 8] [--reps 5]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/exp_contours.py --reps 1             (k_ct_count / k_ct_scan / k_ct_emit)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import model_support  # noqa: E402,F401  (the repository root and the model directories on sys.path)


def terrain_heights(G, seed=20261016):
    rng = np.random.default_rng(seed)
    x = np.linspace(-1.5, 1.5, G, dtype=np.float64)
    X, Z = np.meshgrid(x, x)
    h = np.zeros((G, G))
    for _ in range(24):                                       # hills
        cx, cz, r, a = rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(0.1, 0.5), rng.uniform(-0.3, 0.5)
        h += a * np.exp(-((X - cx) ** 2 + (Z - cz) ** 2) / (r * r))
    for _ in range(8):                                        # ridges
        kx, kz, ph, a = rng.uniform(-9, 9), rng.uniform(-9, 9), rng.uniform(0, 6.28), rng.uniform(0.01, 0.05)
        h += a * np.sin(kx * X + kz * Z + ph)
    return h.astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--levels", type=int, nargs="+", default=[20, 200])
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args(argv)
    import torch
    import contour_model as cm
    import vulkan_forge_amd as vf
    from vulkan_forge_amd import cabi
    W, H = 1920, 1080
    spec = __import__("importlib.util").util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = __import__("importlib.util").util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    poses = np.stack([bench.look_at_uniforms(W, H, (3.0 * np.cos(t), 2.0, 3.0 * np.sin(t))) for t in np.linspace(0, 2 * np.pi, a.poses, endpoint=False)])
    lut = vf.colormap_rgba8("viridis")
    style = dict(width_px=1.0, rgba=(0, 0, 0, 255))
    results = {"frame": [W, H], "poses": a.poses, "reps": a.reps, "cases": []}
    first = None
    for G in a.grids:
        h = terrain_heights(G)
        for nl in a.levels:
            made = {}
            for key in ("plain", "contours", "lines"):
                t = cabi.Terrain(W, H, G, lut, share_ctx=first)
                first = first or t
                t.set_height(h)
                t.set_uniforms(poses[0])
                made[key] = t
            lo, hi = made["contours"].height_bounds()
            levels = np.linspace(lo, hi, nl + 2, dtype=np.float64)[1:-1].astype(np.float32)
            # (a) add time; a first call on a scratch handle takes the one-off costs (code objects, first allocations) out of both routes
            warm = cabi.Terrain(W, H, G, lut, share_ctx=first)
            warm.set_height(h)
            warm.set_uniforms(poses[0])
            warm.add_contours(levels[:2], join=1, **style)
            warm.add_lines(np.zeros((2, 3), np.float32), np.array([0, 2], np.uint32), cap=0, drape=True, **style)
            warm.close()
            t0 = time.perf_counter()
            _, nseg = made["contours"].add_contours(levels, join=1, **style)
            gpu_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            surf = cm.surface(h, G)
            t1 = time.perf_counter()
            recs, nmodel = cm.extract(surf, cm.spacing_of(poses[0]), levels, join="none", bracket=True, **style)
            t2 = time.perf_counter()
            coords = np.empty((2 * nmodel, 3), np.float32)
            coords[0::2], coords[1::2] = recs["p0"], recs["p1"]
            offsets = np.arange(0, 2 * nmodel + 1, 2, dtype=np.uint32)
            t3 = time.perf_counter()
            made["lines"].add_lines(coords, offsets, cap=0, drape=True, **style)
            t4 = time.perf_counter()
            assert nmodel == nseg, (nmodel, nseg)
            host = {"surface_ms": (t1 - t0) * 1e3, "extract_ms": (t2 - t1) * 1e3, "pack_ms": (t3 - t2) * 1e3, "add_lines_ms": (t4 - t3) * 1e3}
            host_ms = sum(host.values())
            # (b) frame time
            stream = torch.cuda.ExternalStream(first.stream_handle())
            outs = [torch.empty(H * W * 4, dtype=torch.uint8, device="cuda") for _ in range(a.poses)]
            ptrs = [o.data_ptr() for o in outs]
            for t in made.values():
                t.render_batch(poses, ptrs, stream.cuda_stream)
            torch.cuda.synchronize()
            ms = {k: [] for k in made}
            order = list(made)
            for r in range(a.reps):
                for key in order[r % 3:] + order[:r % 3]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    made[key].render_batch(poses, ptrs, stream.cuda_stream)
                    e1.record(stream)
                    e1.synchronize()
                    ms[key].append(e0.elapsed_time(e1) / a.poses)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            spread = {k: float(max(v) - min(v)) for k, v in ms.items()}
            case = {"grid": G, "levels": nl, "segments": int(nseg), "add_contours_ms": gpu_ms, "host_route_ms": host_ms, "host_route": host,
                    "frame_ms": med, "frame_ms_spread": spread, "samples_ms": ms}
            results["cases"].append(case)
            print(f"grid {G}, {nl} levels: {nseg} segments; add_contours {gpu_ms:.2f} ms, host route {host_ms:.1f} ms "
                  f"(surface {host['surface_ms']:.1f}, extract {host['extract_ms']:.1f}, pack {host['pack_ms']:.1f}, add_lines {host['add_lines_ms']:.1f}); "
                  f"frame {med['plain']:.3f} ms plain, {med['contours']:.3f} ms contours, {med['lines']:.3f} ms add_lines "
                  f"(max - min of the runs {spread['plain']:.3f} / {spread['contours']:.3f} / {spread['lines']:.3f})", flush=True)
            for t in made.values():
                if t is not first:
                    t.close()
    print(json.dumps(results, default=float))


if __name__ == "__main__":
    main()
